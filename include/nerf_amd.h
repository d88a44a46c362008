/*
 * nerf_amd.h -- C-ABI of libnerf_amd.so: the MI355X (gfx950) native NeRF ray-march hot path.
 *
 * The reference (Enigmatisms/NeRF) has no FFI layer: its hot path is plain Python/torch functions
 * (SURVEY.md section 8b).  This header declares, one entry point per reference callee, what a
 * maintainer of the reference would bind from Python (ctypes stub: INTEGRATION.md) to replace the
 * torch expressions with the hand-written HIP kernels.  Citations are file:line under the
 * reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 (or int64 where stated) unless
 *     marked "host"; no torch types cross this boundary;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     asynchronous on that stream, nothing synchronises the device;
 *   - every function returns 0 on success, a negative NERF_AMD_E* code otherwise;
 *     nerf_amd_last_error() returns a host string describing the last failure of the calling thread;
 *   - inputs are never written; outputs never alias inputs.
 */
#ifndef NERF_AMD_H
#define NERF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_AMD_OK            0
#define NERF_AMD_EINVAL       -1   /* bad argument (NULL pointer, unsupported size)            */
#define NERF_AMD_EUNSUPPORTED -2   /* a configuration the HIP kernels are not instantiated for */
#define NERF_AMD_EHIP         -3   /* a HIP runtime call failed (see nerf_amd_last_error)      */

/* arithmetic of the MLP matrix products */
#define NERF_AMD_F32   0   /* v_mfma_f32_32x32x2_f32: exact fp32 products + fp32 accumulate (parity mode, <=1e-4) */
#define NERF_AMD_BF16  1   /* v_mfma_f32_32x32x16_bf16: bf16 operands, fp32 accumulate (throughput mode)          */
/* NERF_AMD_BF16 arithmetic with the TRAINING DUMPS of the 256-wide hidden layers (activations written by nerf_amd_*_forward_train, deltas
 * written by nerf_amd_*_backward_chain, both read by nerf_amd_*_weight_grads) stored as OCP e4m3 with one power-of-two scale per sample and
 * 16-feature K group: 288 B instead of 512 B per sample and layer in each of the four passes over a dump.  Accepted by exactly those entry
 * points and nerf_amd_train_dump_bytes / nerf_amd_weight_grads_workspace_bytes (pack with NERF_AMD_BF16); encodings and head deltas stay bf16. */
#define NERF_AMD_BF16_F8 2

/* which network a packed weight blob belongs to */
#define NERF_AMD_NET_PROPOSAL 0    /* ProposalNetwork(10, 256)        addtional.py:53-96  */
#define NERF_AMD_NET_MIP      1    /* MipNeRF(10, 4, 256)             mip_model.py:14-60  */
#define NERF_AMD_NET_REF      2    /* RefNeRF(10, 4, 128, 256, 256)   ref_model.py:16-66  */
/* ProposalNetwork(10, 128) -- the reference's class default (addtional.py:61) and `--prop_net_width 128` (procedures.py:176): its own packed
 * layout (five tensors in their 128-wide shapes) and a narrow-tile kernel at a quarter of the 256-wide MACs.  Forward / render only: a blob
 * packed for this network is passed as `packed_prop` together with NERF_AMD_PROP_W128 OR-ed into the call's `precision` argument
 * (nerf_amd_proposal_forward, nerf_amd_render_rays, nerf_amd_render_rays_ref).  Training a narrow network runs the 256-wide kernels on
 * zero-padded tensors (exactly the same function). */
#define NERF_AMD_NET_PROPOSAL_128 3
#define NERF_AMD_PROP_W128 0x100   /* layout flag in `precision`: packed_prop is a NERF_AMD_NET_PROPOSAL_128 blob */
/* MipNeRF(10, 4, 128) -- `--nerf_net_width 128` (procedures.py:177): the eleven tensors in their own shapes (lin_block1 128 wide, lin_block2.0
 * (128, 191), lin_block2.4 (256, 128), the heads as at width 256), a narrow-tile kernel at a third of the 256-wide MACs.  Forward / render with
 * the point PE only: NERF_AMD_FINE_W128 in `precision` of nerf_amd_mip_forward / nerf_amd_render_rays (not with the integrated PE). */
#define NERF_AMD_NET_MIP_128 4
#define NERF_AMD_FINE_W128 0x200   /* layout flag in `precision`: the fine-network blob is a NERF_AMD_NET_MIP_128 blob */

/* density activation applied inside sigma->alpha (nerf_base.py:82 `density_act`) */
#define NERF_AMD_ACT_RELU     0
#define NERF_AMD_ACT_IDENTITY 1    /* RefNeRF passes `lambda x: x` (ref_model.py:26)          */
#define NERF_AMD_ACT_SOFTPLUS 2

const char* nerf_amd_last_error(void);
int         nerf_amd_version(void);                       /* 100*major + minor */
int         nerf_amd_device_info(int* n_cu, int* arch_is_gfx950);

/* ------------------------------------------------------------------------------------------------
 * Where the samples of an MLP launch come from.  Three sources, so that positions never have to be
 * materialised in HBM on the render path:
 *   mode 0  points in memory        pts (M, pts_stride): xyz at [0:3], raw direction at [3:6]
 *                                   (MipNeRF.forward input, mip_model.py:41; ProposalNetwork.forward
 *                                   input, addtional.py:88)
 *   mode 1  rays + depths           x = o + z*d  (NeRF.length2pts nerf_base.py:53-56;
 *                                   procedures.py:66).  rays (N,6) = [o|d]; depth of sample s on ray n:
 *                                   z[n*z_stride + s]                         if z  != NULL
 *                                   z_base[s] + u[n*S + s] * z_jitter          otherwise (stratified
 *                                   draw of procedures.py:65 / utils.py:89 fused in); with u == NULL too
 *                                   the uniform is drawn in the kernel: Philox4x32-10 keyed by rng_seed,
 *                                   a pure function of (ray n + rng_ray_offset, s) -- see below
 *   mode 2  camera + depths         like mode 1 with o = pose[:,3] and d = R.((col-W/2+.5)/fx,
 *                                   (H/2-row+.5)/fy, -1) generated in-kernel for ray n = row*W + col
 *                                   (procedures.py:43-51)
 * M = total samples = N*S in modes 1/2.
 * ARGUMENT DOMAIN OF THE ENCODING (a contract of every entry point that encodes a position: the MLP forwards and renders,
 * nerf_amd_positional_encoding, nerf_amd_ipe_feature*, nerf_amd_encode_rows): the octave-(L-1) argument 2^(L-1) x of every ENCODED
 * coordinate must satisfy |2^(L-1) x| <= 2^21, i.e. |x| <= 4096 at L = 10 -- with disparity spacing out to far = 1000 and |d| <= 3 the
 * largest argument is 1.54e6.  Inside the domain each sine / cosine is within 4 * 2^-24 of the exact function of the fp32 argument
 * (tests/encoding_ref.py); beyond it the range reduction loses accuracy gradually and nothing is promised.  With the scene contraction
 * on, the encoded coordinate is the contracted one (|x| < 2): any finite position is inside the domain.  No field of this descriptor
 * bounds far or |d|, so keeping un-contracted scenes inside the domain is the caller's part.
 * ------------------------------------------------------------------------------------------------ */
#define NERF_AMD_CONTRACT_GAUSSIAN 2 /* nerf_amd_samples.contract: contract the frustum mean AND its covariance (integrated PE) */
typedef struct nerf_amd_samples {
    int32_t      mode;
    int32_t      S;            /* samples per ray (modes 1, 2)                 */
    int64_t      M;            /* total number of samples                      */
    const float* pts;          /* mode 0                                       */
    int32_t      pts_stride;   /* mode 0: floats per sample (3 or 6)           */
    int32_t      z_stride;     /* modes 1/2: floats between rays in z          */
    const float* rays;         /* mode 1: (N, 6)                               */
    const float* z;            /* modes 1/2 or NULL                            */
    const float* z_base;       /* (S) when z == NULL                           */
    const float* u;            /* (N, S) uniforms when z == NULL               */
    float        z_jitter;     /* scale of u when z == NULL                    */
    int32_t      H, W;         /* mode 2                                       */
    float        fx, fy;       /* mode 2: x is divided by fx, y by fy          */
    float        pose[12];     /* mode 2: row-major 3x4 camera-to-world (host) */
    int32_t      contract;     /* != 0: Mip-NeRF 360 scene contraction of the sample POSITION before it is encoded
                                  (Barron et al. 2022, eq. 10): x -> x if |x| <= 1 else (2 - 1/|x|) x/|x|.  Not in the
                                  reference (BASELINE config 5 only); occupies former tail padding, 0 = off.
                                  NERF_AMD_CONTRACT_GAUSSIAN (2; meaningful with `ipe` on the MipNeRF kernels): the frustum's whole
                                  Gaussian goes through the linearised contraction (eq. 11-14): mu' = f(mu), Sigma' = J Sigma J^T,
                                  and the encoder attenuates with diag Sigma' -- with 1 only the mean is contracted and the
                                  covariance stays metric.  Inside the unit ball both are the same bits.  Every point-encoding
                                  kernel (proposal, Ref-NeRF, MipNeRF without `ipe` inside a render) reads 2 as 1; the entry
                                  points refuse any other value, and 2 on a bare MipNeRF descriptor without `ipe`.  */
    int32_t      ipe;          /* != 0 (modes 1 with z only, MipNeRF kernels): integrated positional encoding.  Sample s of ray n is the
                                  conical frustum between z[n*z_stride+s] and z[n*z_stride+s+1] (so z rows hold S+1 depths); the network
                                  input is [mu | ipe_feature(mu, diag Sigma)] (mip_methods.py:15-58) instead of [x | PE(x)].        */
    float        ipe_radius;   /* pixel radius r of coneParameters (mip_methods.py:15)                                              */
    const float* ipe_dir_norm; /* DEVICE pointer to one float: norm of the whole (N,3) direction tensor (mip_methods.py:31;
                                  nerf_amd_dirs_norm)                                                                              */
    uint64_t     rng_seed;     /* in-kernel uniforms (z == NULL and u == NULL; modes 1, 2): the stratified draw of sample s of ray n is    */
    int64_t      rng_ray_offset; /* word 0 of Philox4x32-10(key = rng_seed, counter = (n + rng_ray_offset [64 bit], s, 'RS' = 0x5253)),
                                  top 24 bits * 2^-24.  The reference draws these on the CPU generator (procedures.py:65, utils.py:89);
                                  the counter form needs no tensor, replays from the seed, and is independent of how rays are batched.
                                  nerf_amd_resample / nerf_amd_render_rays regenerate the same values from the same (seed, offset). */
} nerf_amd_samples;

/* ------------------------------------------------------------------------------------------------
 * Weights.  The kernels stream MFMA-fragment-ordered weights through LDS; packing turns the
 * reference's nn.Linear tensors ((out,in) row-major fp32, state_dict order below) into that stream.
 * Re-pack after every optimiser step (a few microseconds).
 *   proposal: layers.{0,2,4,6,8}                                   (addtional.py:67-71)
 *   mip     : lin_block1.{0,2,4,6}, lin_block2.{0,2,4}, bottle_neck.0, opacity_head.0,
 *             rgb_layer.{0,2}                                        (mip_model.py:19-37)
 *   ref     : spa_block1.{0,2,4,6}, spa_block2.{0,2,4,6}, bottle_neck, heads, dir_block1.{0,2,4,6},
 *             dir_block2.{0,2,4,6}, spec_rgb_head.0, ide_table                       (ref_model.py:31-62)
 *             where `heads` is the (11,256) row-concatenation [norm_col_tint_head[0:3], rho_tau_head[0:1],
 *             norm_col_tint_head[3:6], rho_tau_head[1:2], norm_col_tint_head[6:9]] (+ its (11) bias), and
 *             `ide_table` is the (9,19) fp32 coefficient matrix of ref_func.py:60-74 passed in the `weights`
 *             slot (its `biases` slot is ignored and may repeat any valid pointer).
 * `weights` / `biases` are HOST arrays of DEVICE pointers in that order.
 * ------------------------------------------------------------------------------------------------ */
size_t nerf_amd_packed_bytes(int net, int precision);
int    nerf_amd_pack_weights(int net, int precision, const float* const* weights, const float* const* biases,
                             int n_tensors, void* packed, void* stream);

/* ProposalNetwork.forward (addtional.py:88-96): density (M) fp32, no activation. */
int nerf_amd_proposal_forward(const void* packed, int precision, const nerf_amd_samples* src,
                              float* density, void* stream);
/* MipNeRF.forward (mip_model.py:41-60): rgbo (M, 4) = [sigmoid rgb | raw sigma]. */
int nerf_amd_mip_forward(const void* packed, int precision, const nerf_amd_samples* src,
                         float* rgbo, void* stream);
/* (added after ABI 125; additive) rays (N,6) -> table (N, 32) bf16: for each ray the direction columns of rgb_layer.0's input, PE4(d/|d|) in
 * MFMA B-operand order: [lane half 0: K groups 0, 1 | lane half 1: K groups 0, 1], 16 bytes each.  table: 16-byte aligned.  This is what
 * nerf_amd_mip_forward computes once per ray itself on ray descriptors (mode 1 with explicit z, no contraction, no integrated PE) whose S
 * is a multiple of 64 -- there the NERF_AMD_BF16 kernel takes a wave's 64 samples as one ray; before it writes them, it uses each 64-sample
 * block of `rgbo` as scratch for that block's 64 bytes of encoding, so no workspace is needed.  Same bits as the per-sample kernel. */
int nerf_amd_direction_table(const float* rays, int64_t N, void* table, void* stream);

/* MipNeRF.forward + NeRF.render fused (mip_model.py:41-60 + nerf_base.py:91-113, mul_norm = True, relu density): the
 * (N,S,4) network output stays on chip; the last wavefront of each ray composites it.  `src` must be mode 1 (rays + z) with
 * S in {32, 64, 128}.  Outputs rgb (N,3), depth (N) or NULL, weights (N,S) or NULL.  256-wide blobs only: NERF_AMD_FINE_W128 in
 * `precision` is refused (EUNSUPPORTED) -- a NERF_AMD_NET_MIP_128 blob takes nerf_amd_mip_forward + nerf_amd_composite. */
int nerf_amd_mip_forward_composite(const void* packed, int precision, const nerf_amd_samples* src, int white_bkg,
                                   float near, float far, float* rgb, float* depth, float* weights, void* stream);

/* RefNeRF.forward in eval mode (ref_model.py:68-106): rgbo (M,4) = [rgb | raw density], normal (M,3) (NULL to skip).  Samples need a
 * direction (pts_stride >= 6 in mode 0).  ref_flags: NERF_AMD_REF_SRGB = the module's use_srgb (ref_model.py:100-102:
 * rgb = linear_to_srgb(specular + sigmoid(diffuse - log 3))), 0 = ref_model.py:104-105.  The same flag goes to every Ref-NeRF entry point. */
#define NERF_AMD_REF_SRGB 1
int nerf_amd_ref_forward(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags,
                         float* rgbo, float* normal, void* stream);
/* Training-mode forward (ref_model.py:84-85): the same kernel with the bottle-neck perturbation `bn_noise` (M,128), which the
 * caller draws (torch.normal(0, perturb_bottle_neck_w)) so that the backward can re-evaluate with the same noise. */
int nerf_amd_ref_forward_train(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, const float* bn_noise,
                               float* rgbo, float* normal, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sampling / compositing kernels (one 64-lane wavefront per ray; HBM-bound).
 * ------------------------------------------------------------------------------------------------ */

/* positional_encoding (nerf_helper.py:38-48): x (M,3) -> out (M, 6L) = [sin 2^0 x, cos 2^0 x, sin 2^1 x, ...] */
int nerf_amd_positional_encoding(const float* x, int64_t M, int L, float* out, void* stream);

/* ipe_feature with its helpers coneParameters / coneMeanCov / multFreq (mip_methods.py:15-58): z (N, S+1) depths, rays (N,6),
 * L frequency levels, pixel radius r -> feat (N, S, 6L) = per level [sin(2^l mu) e^(-4^l diag/2) xyz | cos(...) xyz], mu (N,S,3) or NULL,
 * mu_t (N,S) or NULL.  `dir_norm` is a DEVICE pointer to the norm of the whole (N,3) direction tensor (the reference's `.norm()`
 * without a dim, :31) -- nerf_amd_dirs_norm computes it.  The reference never calls ipe_feature from its entry scripts
 * (SURVEY.md 8a row 12); golden G12 pins the function. */
int nerf_amd_ipe_feature(const float* z, const float* rays, int64_t N, int S, int L, float r, const float* dir_norm,
                         float* feat, float* mu, float* mu_t, void* stream);
/* (ABI 125) the same with the Mip-NeRF 360 scene contraction of the frustum MEAN before the lift (the diagonal covariance stays metric):
 * what the fused kernels' sample fetch computes for `ipe` + `contract` together (BASELINE configs[2] + configs[4]); `mu` receives the
 * CONTRACTED mean.  Not in the reference (mip_methods.py has no contraction): the build's own definition, oracle.ipe_feature(contracted=True).
 * The layer-by-layer route of networks larger than the compiled shapes encodes with it. */
int nerf_amd_ipe_feature_contracted(const float* z, const float* rays, int64_t N, int S, int L, float r, const float* dir_norm,
                                    float* feat, float* mu, float* mu_t, void* stream);
/* (ABI 125, additive) the same with the whole Gaussian contracted (Mip-NeRF 360 eq. 11-14; nerf_amd_samples.contract =
 * NERF_AMD_CONTRACT_GAUSSIAN): mu' = contract(mu) as above, and the attenuation reads diag(J Sigma J^T) with
 * Sigma = (var_t - var_r / dir_norm) d d^T + var_r I and J the contraction's Jacobian at the metric mean.  Frusta
 * whose metric mean lies inside the unit ball give the bits of nerf_amd_ipe_feature_contracted. */
int nerf_amd_ipe_feature_gaussian(const float* z, const float* rays, int64_t N, int S, int L, float r, const float* dir_norm,
                                  float* feat, float* mu, float* mu_t, void* stream);
/* coneParameters (mip_methods.py:15-23): z (N, S+1) -> mu_t, sigma_t^2, sigma_r^2, each (N, S). */
int nerf_amd_cone_parameters(const float* z, int64_t N, int S, float r, float* mu_t, float* var_t, float* var_r, void* stream);
/* sqrt(sum of squares) of the direction halves of rays (N,6) -> out (1 float on the device); fp64 accumulation, fixed order. */
int nerf_amd_dirs_norm(const float* rays, int64_t N, float* out, void* stream);

/* Ray table of render_image (procedures.py:43-51,64): rays (N, 6) = [pose[:,3] | R.c] for pixels
 * n = row*W + col in [ray_offset, ray_offset+N); `pose_host` is a HOST row-major 3x4. */
int nerf_amd_generate_rays(const float* pose_host, int H, int W, float fx, float fy, int64_t ray_offset, int64_t N,
                           float* rays, void* stream);

/* (added after ABI 125; additive) The camera model: principal point, lens distortion, per-view intrinsics.
 * A camera is a row of NERF_AMD_CAMERA_ROW fp32 values
 *     fx, fy, cx, cy, k1, k2, k3, p1, p2, 0, 0, 0
 * with cx, cy in pixels in COLMAP's convention -- the centre of pixel (col, row) is at (col + 0.5, row + 0.5) -- and the last three
 * entries reserved (a non-zero value there is NERF_AMD_EINVAL).  The distorted image-plane point of a pixel, with true divisions:
 *     xd = (((float)col + 0.5f) - cx) / fx        yd = (((float)row + 0.5f) - cy) / fy
 * The forward model (OpenCV / COLMAP), r2 = x^2 + y^2, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)):
 *     xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2)      yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2)
 * The undistorted (xu, yu) solves it for (x, y): NERF_AMD_CAMERA_NEWTON_STEPS steps of Newton's method from (xd, yd) with the analytic
 * 2x2 Jacobian, every one taken (no convergence test), except that a step whose |determinant| is below NERF_AMD_CAMERA_DET_EPS is
 * skipped.  When all five coefficients are zero no step is taken: (xu, yu) = (xd, yd) exactly.  The ray is o = pose[:,3],
 * d = R.(xu, -yu, -1): the cameras look down -z with y up; converting a COLMAP world-to-camera pose is the caller's job.
 * The ray table of nerf_amd_generate_rays adds its 0.5 after the flip, so it IS this model at cx = W/2, cy = H/2 + 1, and the training
 * samplers are it at cx = W/2 (integer halves), cy = H/2 + 1: every numerator is a small integer or half, exact in fp32, and those
 * cameras reproduce today's rays bit for bit.  The steps suffice (the fp64 iteration's residual is below 1e-12) where the forward model's
 * Jacobian determinant stays well away from zero over the image -- above 0.3 for the cameras tests/test_camera_host.py walks through;
 * tests/camera_ref.py is the fp64 specification and derives the fp32 bounds. */
#define NERF_AMD_CAMERA_ROW 12
#define NERF_AMD_CAMERA_NEWTON_STEPS 3
#define NERF_AMD_CAMERA_DET_EPS 1e-6f
/* nerf_amd_generate_rays for one camera row (HOST, validated: finite, fx, fy > 0, zero tail): same indexing, rays (N, 6). */
int nerf_amd_generate_rays_camera(const float* pose_host, int H, int W, const float* camera_host, int64_t ray_offset, int64_t N, float* rays,
                                  void* stream);

/* NeRF.length2pts (nerf_base.py:53-56): out (N, S, 6) = [o + z d | d]. */
int nerf_amd_length2pts(const float* rays, const float* z, int64_t N, int S, float* out, void* stream);

/* ProposalNetwork.get_weights (addtional.py:100-107) / NeRF.getNormedWeight (nerf_base.py:80-86):
 * sigma (N,S), z (N,S), dirs (N,3) or NULL (NULL = z already scaled) -> w (N,S). */
int nerf_amd_sigma_to_weights(const float* sigma, const float* z, const float* dirs, int64_t N, int S, int act,
                              float* w, void* stream);

/* maxBlurFilter (mip_methods.py:61-66): w (N,S) -> out (N,S). */
int nerf_amd_max_blur(const float* w, int64_t N, int S, float alpha, float* out, void* stream);

/* inverseSample (utils.py:34-44) + sample_pdf (utils.py:108-133) with the uniforms explicit:
 * w (N,C), z (N,C), u (N,K) -> z_out (N,K) [sorted when sort!=0], below (N,K) int64 (NULL to skip). C <= 256.
 * The sampling contract, which this entry, nerf_amd_sample_pdf and every fused resampling entry (nerf_amd_resample,
 * nerf_amd_warped_resample, the render requests) share:
 *   cdf        [0 | cumsum((w + 1e-5) / sum(w + 1e-5))] in fp32, bit for bit torch's CPU result (the sum in ATen's order, the running sum
 *              in fp64 rounded per element); inds = #{j: cdf[j] <= u} (searchsorted, right=True)
 *   indices    below = max(inds - 1, 0), above = min(inds, nb - 1), nb = the number of bin edges; u >= cdf[nb - 1] gives below == above
 *   sample     bins[below] + t (bins[above] - bins[below]), t = (u - cdf[below]) / d, d = cdf[above] - cdf[below], d < 1e-5 -> 1;
 *              separate fp32 operations in this order, IEEE division
 *   sort != 0  the samples ASCENDING BY VALUE for every input -- the stable sort of the raw fp32 samples, like torch.sort -- and
 *              `below` permuted with them (equal values may come in any order).  Over ascending bin edges that is the order of the
 *              uniforms except where a sample exceeds its bin's upper edge by an ulp of fp32 rounding; such rays, and rays whose bin
 *              edges descend, are sorted by value all the same. */
int nerf_amd_inverse_sample(const float* w, const float* z, const float* u, int64_t N, int C, int K, int sort,
                            float* z_out, int64_t* below, void* stream);

/* sample_pdf (utils.py:108-133): bins (N,B), weights (N,B-1), u (N,K) -> samples (N,K), below/above (N,K) int64 or NULL. */
int nerf_amd_sample_pdf(const float* bins, const float* weights, const float* u, int64_t N, int B, int K, float* samples,
                        int64_t* below, int64_t* above, void* stream);

/* Training twin of the ray table (validSampler, utils.py:78-85): integer pixel coords (N,2) int64 =
 * (col - W//2, H//2 - row) from randomFromOneImage -> rays (N,6). */
int nerf_amd_pixel_rays(const float* pose_host, float fx, float fy, const int64_t* coords, int64_t N, float* rays, void* stream);

/* validSampler (utils.py:72-94) with every random number drawn in the kernel: N rays through uniformly drawn pixels of
 * the flattened pixel table rgbs (n_pixels,3) / coords (n_pixels,2) int64 of randomFromOneImage, their ground-truth colours rgb (N,3),
 * rays (N,6) = [pose[:,3] | R.c], and -- when pts / lengths are given -- C stratified depths lengths (N,C) = linspace(near, far - res, C)
 * + u res, res = (far-near)/C, with the positions pts (N,C,3).  Uniforms: Philox4x32-10 keyed by rng_seed; pixel index of ray n =
 * floor(n_pixels * u64 / 2^64) of counter (n, 0, 'IX'), depth uniform = word s&3 of counter (n, s>>2, 'TS'). */
int nerf_amd_sample_training_rays(const float* rgbs, const int64_t* coords, int64_t n_pixels, const float* pose_host, float fx, float fy,
                                  float near, float far, int64_t N, int C, uint64_t rng_seed, float* pts, float* lengths, float* rgb,
                                  float* rays, void* stream);
/* The same with the camera pose (3,4) and the seed read from DEVICE memory at run time: nothing about the step is baked into the launch
 * arguments, so a training step captured once in a hipGraph sees a new image pose and fresh random numbers on every replay
 * (nerf_amd/training.py).  nerf_amd_advance_seed replaces *seed_dev by an unrelated key (one thread; put it at the end of the step);
 * nerf_amd_philox_uniforms fills u (N,K) with the inverse-CDF stream of nerf_amd_resample (key = rng_seed, or *seed_dev when given) for
 * callers that keep inverseSample(weights, depths, u) as a separate op (utils.py:34-44, 115). */
int nerf_amd_sample_training_rays_dev(const float* rgbs, const int64_t* coords, int64_t n_pixels, const float* pose_dev, float fx, float fy,
                                      float near, float far, int64_t N, int C, const uint64_t* seed_dev, float* pts, float* lengths,
                                      float* rgb, float* rays, void* stream);
int nerf_amd_philox_uniforms(float* out, int64_t N, int K, uint64_t rng_seed, const uint64_t* seed_dev, void* stream);
/* (added after ABI 125; additive) The same batch drawn uniformly over ALL training pixels of a scene in one launch: images (V,3,H,W) fp32
 * planar and poses (V,3,4) fp32, both on the device and read in place (no pixel table, no coordinate table).  view_ids (K,) int64 on the
 * device selects K of the V views (NULL: views 0..K-1; pass K = V for the whole stack; an entry outside [0, V) reads nothing: its rays come out NaN with index -1);
 * the window x0 <= col < x1, y0 <= row < y1 is the centre crop of randomFromOneImage (0, W, 0, H = the whole image).  With
 * wp = (y1-y0)(x1-x0) and P = K wp, ray n draws cell = floor(P * u64 / 2^64) from the SAME word of the same counter (n, 0, 'IX') as
 * nerf_amd_sample_training_rays, then k = cell / wp, r = cell % wp, row = y0 + r / (x1-x0), col = x0 + r % (x1-x0), v = view_ids ?
 * view_ids[k] : k -- all in 64-bit.  rgb (N,3) = images[v, :, row, col]; rays (N,6) = [poses[v][:,3] | R_v.(cx, cy, -1)] with
 * cx = ((float)(col - W/2) + 0.5f) / fx, cy = ((float)(H/2 - row) + 0.5f) / fy (integer halves, the coordinate table's values);
 * index (N) int64 = (v H + row) W + col, or NULL to skip; lengths (N,C) / pts (N,C,3) as in nerf_amd_sample_training_rays (stream 'TS'),
 * skipped when lengths is NULL or C == 0 (pts without lengths is an error).  Key: rng_seed, or *seed_dev (device) when given.
 * With K = 1 the outputs are bit-identical to nerf_amd_sample_training_rays_dev on randomFromOneImage(images[v]) with the same seed: the
 * window is enumerated row-major like the table. */
int nerf_amd_sample_scene_rays(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0,
                               int x1, int y0, int y1, float fx, float fy, float near, float far, int64_t N, int C, uint64_t rng_seed,
                               const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index, void* stream);
/* (added after ABI 125; additive) nerf_amd_sample_scene_rays with per-view cameras: `cameras` (V, NERF_AMD_CAMERA_ROW) fp32 on the DEVICE,
 * row v the camera of view v (the model above), read when the kernel runs -- the host never sees its values, so a captured step replays
 * with whatever the table then holds.  rays (N,6) = [poses[v][:,3] | R_v.(xu, -yu, -1)] of pixel (col, row) under cameras[v]; every
 * draw, the window, view_ids, index, rgb, lengths and pts are nerf_amd_sample_scene_rays' own (the same Philox words).  With every row
 * (fx, fy, W/2, H/2 + 1, 0 ...) in integer halves the outputs are bit-identical to nerf_amd_sample_scene_rays. */
int nerf_amd_sample_scene_rays_camera(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0,
                                      int x1, int y0, int y1, const float* cameras, float near, float far, int64_t N, int C, uint64_t rng_seed,
                                      const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index,
                                      void* stream);
/* (ABI 121) Either Philox stream of the render kernels as a tensor, for rows that are GLOBAL rays ray_offset .. ray_offset + N - 1: the
 * uniforms the reference draws per tile with torch.rand (procedures.py:65 stratified jitter -> NERF_AMD_PHILOX_STRAT, K <= 64;
 * utils.py:115 inverse-CDF -> NERF_AMD_PHILOX_INV), bit-identical to what nerf_amd_render_rays draws in place for the same seed and ray
 * index -- so a network outside the fused kernels' shapes (the layer-by-layer route) renders with the same random numbers. */
#define NERF_AMD_PHILOX_INV 0
#define NERF_AMD_PHILOX_STRAT 1
int nerf_amd_philox_stream(float* out, int64_t N, int K, uint64_t rng_seed, const uint64_t* seed_dev, int64_t ray_offset, int stream_id,
                           void* stream);
int nerf_amd_advance_seed(uint64_t* seed_dev, void* stream);

/* Stratified depths and points (utils.py:87-90, procedures.py:65-66): z = z_base[s] + u*z_jitter (N,S);
 * pts (N,S,3) = o + d*z, or NULL to skip. */
int nerf_amd_stratified_points(const float* rays, const float* z_base, const float* u, float z_jitter, int64_t N, int S,
                               float* z_out, float* pts, void* stream);

/* Fused proposal resampling of the render/train loop (procedures.py:68-70, train.py:169-172):
 * density -> [softplus] -> get_weights(|d| scaling, relu) -> maxBlur(alpha) -> inverse sample (sorted).
 * Depths as in nerf_amd_samples (z, or z_base + u_strat*z_jitter).  dirs row n at dirs[n*dirs_stride .. +3]
 * (pass rays+3 with stride 6).  Optional outputs (NULL to skip): w_prop (N,C), below (N,K) int64, z_coarse (N,C).
 * A NULL u_strat (with z == NULL) / a NULL u_inv is drawn in the kernel from (rng_seed, ray + rng_ray_offset) exactly like
 * nerf_amd_samples describes; words 1..3 of the same blocks are the inverse-CDF draws: u_inv(n, k), k = 192 b + r (r < 192), is word
 * 1 + r/64 of Philox4x32-10(key = rng_seed, counter = (n + rng_ray_offset, 64 b + r%64, 'RS')) -- at the render shapes one block per
 * (ray, lane) carries everything that lane needs. */
int nerf_amd_resample(const float* density, const float* z, const float* z_base, const float* u_strat, float z_jitter,
                      const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K,
                      int softplus_density, float blur_alpha, uint64_t rng_seed, int64_t rng_ray_offset,
                      float* z_fine, int64_t* below, float* w_prop, float* z_coarse, void* stream);

/* NeRF.render (nerf_base.py:91-113).  rgbo (N,S,4), z (N,z_stride) [first S used], dirs as above.
 * flags: bit0 mul_norm, bit1 white_bkg.  density = act(sigma + sigma_shift) (sigma_shift 0.5 + softplus is
 * the Ref-NeRF render path, procedures.py:74).  Outputs: rgb (N,3), weights (N,S) or NULL, depth (N) or NULL
 * ((sum w z - near)/(far-near)), normal_img (N) or NULL when normal (N,S,3) and cam_dir (3, device) given. */
int nerf_amd_composite(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride,
                       int64_t N, int S, int flags, int act, float sigma_shift, float near, float far,
                       const float* normal, const float* cam_dir,
                       float* rgb, float* weights, float* depth, float* normal_img, void* stream);

/* The depth sort of NeRF.coarseFineMerge (nerf_base.py:59-73) for the render path (procedures.py:72): z_fine (N,K) and z_coarse
 * (N,C) -> z_out (N, K+C-1) = sort(cat(z_fine, z_coarse))[..., :-1].  Both inputs are normally ascending along the last dimension
 * (then this is a merge); a ray whose input is out of order -- stratified depths with a jitter above the bin spacing, n_fine < 63 --
 * is sorted first, so the result always equals the sort.  K + C <= 2048. */
int nerf_amd_merge_depths(const float* z_fine, const float* z_coarse, int64_t N, int K, int C, float* z_out, void* stream);

/* NeRF.coarseFineMerge as the TRAINING loop calls it (nerf_base.py:59-73 with f_inds; train.py:176): z_out as above, plus
 * order (N, K+C) int64 = the stable argsort of cat(z_fine, z_coarse) (fine index i before coarse index K + j among equal depths --
 * what torch.sort's device radix sort returns; the reference hands order[..., :-1] to RefNeRF.coarse_grad_select), and, when
 * f_inds (N,K) int64 is given, all_inds (N, K+C) int64 = gather(cat(f_inds, arange(C)), order) (the bin indices getBounds reads).
 * f_inds / all_inds may be NULL.  K + C <= 1024. */
int nerf_amd_merge_depths_order(const float* z_fine, const float* z_coarse, const int64_t* f_inds, int64_t N, int K, int C, float* z_out,
                                int64_t* order, int64_t* all_inds, void* stream);

/* RefNeRF.coarse_grad_select (ref_model.py:108-117): grads (N,T,D) fp32, sort_inds (N,T) int64 -> out (N,c_pnum,D): the rows of the
 * first c_pnum positions p (ascending) with sort_inds[n,p] >= T - c_pnum -- the reference's boolean mask
 * gather(cat(zeros(T-c), ones(c)), sort_inds) without its data-dependent output size; rows with fewer flagged positions continue with
 * the unflagged ones in order. */
int nerf_amd_coarse_grad_select(const float* grads, const int64_t* sort_inds, int64_t N, int T, int D, int c_pnum, float* out, void* stream);

/* Ref-NeRF's normal losses (ref_model.py:127-143) as one streaming pass + a fixed-order two-stage sum (deterministic):
 *   mode 0  WeightedNormalLoss(size_average=False): out[0] = scale * sum_i w_i (1 - <a_i, b_i>)      (a = d_norm, b = p_norm; scale 1, or 1/M for size_average)
 *   mode 1  BackFaceLoss:                            out[0] = scale * sum_i w_i relu(<a_i, b_i>)      (a = normal, b = ray_d; scale = 1 / M: torch.mean)
 * w (M), a, b (M,3) fp32 contiguous; workspace: NERF_AMD_DOT_LOSS_WORKSPACE_FLOATS floats.
 * Backward: g = d loss / d out (ONE float in device memory, so the call needs no synchronisation) -> d_w (M), d_a, d_b (M,3); any of the
 * three may be NULL. */
#define NERF_AMD_DOT_LOSS_WORKSPACE_FLOATS 512
int nerf_amd_weighted_dot_loss(const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* out, float* workspace, void* stream);
int nerf_amd_weighted_dot_loss_backward(const float* g, const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* d_w,
                                        float* d_a, float* d_b, void* stream);

/* Distortion regularisers, one wavefront per ray (the row staged in LDS in fp32, pair sums in fp64) + a fixed-order two-stage sum
 * (deterministic; no host synchronisation, so capturable).  t (N, S) fp32 contiguous, 2 <= S <= NERF_AMD_DISTORTION_MAX_S depths per row:
 *   mode 0  Regularizer (addtional.py:26-35): w (N, S), rows in any order, M = S - 1 intervals with c_i = (t_i + t_i+1) / 2,
 *           a_i = (w_i + w_i+1) / 2, d_i = t_i+1 - t_i, r_i = sqrt(sum_j (c_i - c_j)^2):
 *           out[0] = scale * ( sum_n sum_ij a_i a_j |c_i - c_j| / r_i / (N M^2)  +  sum_n sum_i d_i a_i^2 / (3 N M) )
 *           -- the reference's two means; a row whose centres coincide (S = 2 among them) gives 0/0 = NaN, as the reference does.
 *   mode 1  Mip-NeRF 360 L_dist (Barron et al. 2022, eq. 15): w (N, S - 1), t = the S sorted interval edges, m_i = interval midpoints:
 *           out[0] = scale / N * sum_n ( sum_ij w_i w_j |m_i - m_j|  +  sum_i w_i^2 (t_i+1 - t_i) / 3 )
 * workspace: NERF_AMD_DISTORTION_WORKSPACE_FLOATS floats.  Backward: g = d loss / d out (ONE float in device memory) -> d_w (the shape of w),
 * d_t (N, S); either may be NULL (not computed).  sgn(0) = 0 in the gradient of |x|, as torch: intervals whose centres tie bit for bit
 * (zero-width intervals from repeated depths) exchange no |x| gradient.  g and scale are multiplied in on the device (in fp64); out[0]
 * does not contain g.  A ray all of whose centres coincide: mode 0 stores NaN in every column of THAT ray's rows of d_w and d_t (and
 * out[0] is NaN), every other ray's rows are unaffected; mode 1 stores exact zeros in its d_w row and the widths' part in d_t.  A
 * gradient entry all of whose terms are exact zeros (zero weights) is stored as an exact zero.  (tests/test_gpu_regularizers.py) */
#define NERF_AMD_DISTORTION_MAX_S 1024
#define NERF_AMD_DISTORTION_WORKSPACE_FLOATS 4096
int nerf_amd_distortion_loss(const float* w, const float* t, int64_t N, int S, int mode, float scale, float* out, float* workspace, void* stream);
int nerf_amd_distortion_loss_backward(const float* w, const float* t, int64_t N, int S, int mode, float scale, const float* g, float* d_w,
                                      float* d_t, void* stream);

/* (added after ABI 125; additive) Mip-NeRF 360's interlevel loss L_prop (Barron et al. 2022, eq. 13), not in the reference: the fine histogram (w, t) is bounded from above
 * by the proposal histogram (w_prop, t_prop) -- each fine weight by the proposal mass whose intervals geometrically overlap its interval.
 * Unlike getBounds + ProposalLoss (bin indices of ONE sampler call) it needs no relation between the two sample sets, so a histogram the
 * fine samples were not drawn from directly can be supervised as well.  All fp32 contiguous, rows ascending, 1 <= M, K <= NERF_AMD_INTERLEVEL_MAX:
 *   w (N, M) fine weights (constants), t (N, M + 1) fine edges, w_prop (N, K), t_prop (N, Kp) with Kp = K + 1 (closed: the K + 1 edges) or
 *   Kp = K (open: the K depths of point samples; interval j = [t_j, t_j+1), the last one open to +inf, as get_weights composites it).
 * With e the K + 1 proposal edges (+inf appended in the open form) and c the exclusive prefix sum of w_prop (c_0 = 0, K + 1 entries):
 *   lo(v) = max{ j : e_j <= v } (0 if none),  hi(v) = min{ j : e_j > v } (K if none),  bound_i = c[hi(t_i+1)] - c[lo(t_i)]
 *   out[0] = scale * sum_n sum_i relu(w_i - bound_i)^2 / (w_i + 1e-8)                   (a sum over rays, eps 1e-8: as ProposalLoss)
 * -- a proposal interval that merely touches a fine one counts as overlapping; a fine interval wholly outside the proposal's span has
 * bound 0.  bounds_out (N, M) may be NULL (not written).  One wavefront per ray, the edge rows and the fp64 prefix sums in LDS; prefix
 * sums, bounds, per-ray partials and the cross-ray sum are fp64 in a fixed order, only the stored values are rounded to fp32
 * (deterministic; no host synchronisation, so capturable).  workspace: NERF_AMD_INTERLEVEL_WORKSPACE_FLOATS floats.
 * Backward: g = d loss / d out (ONE float in device memory) -> d_w_prop (N, K):
 *   d_w_prop[j] = g scale sum_{i : lo(t_i) <= j < hi(t_i+1)} -2 relu(w_i - bound_i) / (w_i + 1e-8)
 * -- the i of one j are a contiguous range (t_i < e_j+1 and t_i+1 >= e_j): two binary searches and a difference of an fp64 prefix sum,
 * no atomics.  The loss is piecewise constant in the edges and w is a constant: there is no other gradient.
 * Settled by tests/test_gpu_regularizers.py: bounds_out of a fine interval outside a closed proposal span is the exact 0 (hi = lo: one
 * prefix entry minus itself), elsewhere the fp32 rounding of an fp64 difference of prefix sums (absolute error ~1e-16 of the row's total
 * weight, which is what a bound ten decades below the total carries); a fine edge that equals a proposal edge bit for bit counts on both
 * sides (`<=` in lo, `>` in hi); d_w_prop[j] of a proposal interval that no fine interval touches is the stored constant 0; a row of M
 * coincident fine edges is M zero-width intervals, nothing special; g and scale are multiplied in on the device, out[0] does not contain g. */
#define NERF_AMD_INTERLEVEL_MAX 1024
#define NERF_AMD_INTERLEVEL_WORKSPACE_FLOATS 2048
int nerf_amd_interlevel_loss(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale,
                             float* out, float* bounds_out, float* workspace, void* stream);
int nerf_amd_interlevel_loss_backward(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp,
                                      float scale, const float* g, float* d_w_prop, void* stream);

/* Measurement aid, no reference counterpart (the roofline's denominator checked on the box): `workgroups` workgroups of four
 * waves (one per SIMD; 160 KiB of LDS each, so one workgroup per CU) issue iters * 64 v_mfma_f32_32x32x16_bf16 per wave and nothing else;
 * timed by the caller, 32 768 flop per MFMA and wave.  mode 0: constant operands (optimistic: the datapath does not toggle); 1: a rotating
 * pool of pseudo-random bf16 A / B register groups (pessimistic); 2: random weights-like A, post-ReLU-like B (half zeros); 3: mode 2 with
 * every A operand read from LDS four fragments ahead and feeding two MFMAs (the weight ring's cadence).  sink: 256 floats (never written
 * in practice). */
int nerf_amd_mfma_stream(int iters, int workgroups, int mode, float* sink, void* stream);

/* getBounds (addtional.py:14-18): w_prop (N,C), below (N,K) int64 -> bounds (N,K-1).
 * bounds_k = sat[below_{k+1} + 1] - sat[below_k] over the summed-area row sat[0 .. C] of w_prop.  Every entry of `below` must lie in
 * 0 ... C - 1 (what the resampling kernels emit), sorted or not; like the reference's torch.gather, which raises outside that range, the
 * forward kernel does not clamp, and an index outside it reads outside the row.  nerf_amd_get_bounds_backward has the same contract. */
int nerf_amd_get_bounds(const float* w_prop, const int64_t* below, int64_t N, int C, int K, float* bounds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training forward of the MLPs: same kernels and results as nerf_amd_{proposal,mip}_forward, and in
 * addition every hidden layer's post-ReLU activations are written to `dump` (nerf_amd_train_dump_bytes bytes, device) in the
 * kernels' fragment order.  nerf_amd_train_dump_to_rows turns one layer of a dump into a row-major (M, n_features) matrix
 * (bf16 for NERF_AMD_BF16, fp32 for NERF_AMD_F32) for the dgrad / wgrad GEMMs.
 * Layers: proposal 0..3 = layers.{0,2,4,6} outputs (256 wide), 4 = the input encoding [x | PE10(x)] in the kernels' slot order;
 * MipNeRF 0..3 = lin_block1.{0,2,4,6}, 4..6 = lin_block2.{0,2,4} (256 wide), 7 = rgb_layer.0 output (128 wide), 8 = the position and
 * direction encodings in slot order (operands of the first-layer / skip-layer / colour-head weight gradients).
 * ------------------------------------------------------------------------------------------------ */
size_t nerf_amd_train_dump_bytes(int net, int precision, int64_t M);
int nerf_amd_proposal_forward_train(const void* packed, int precision, const nerf_amd_samples* src, float* density, void* dump,
                                    void* stream);
int nerf_amd_mip_forward_train(const void* packed, int precision, const nerf_amd_samples* src, float* rgbo, void* dump, void* stream);
int nerf_amd_train_dump_to_rows(const void* dump, int net, int precision, int64_t M, int layer, int n_features, void* out,
                                void* stream);
/* ReLU adjoint of the dgrad chain, in place: delta[i] = act[i] > 0 ? delta[i] : 0 over n elements (bf16 / fp32 as above). */
int nerf_amd_relu_mask(void* delta, const void* act, int precision, int64_t n, void* stream);
/* The same over a (rows, cols) matrix with the bias gradient fused in: `col_sum` receives nerf_amd_relu_mask_bias_partials(...) rows of
 * `cols` fp32 partial column sums of the masked delta (written, not accumulated: no atomics, reproducible); their sum over the rows is
 * the bias gradient.  cols * element size / 4 must divide 256. */
int64_t nerf_amd_relu_mask_bias_partials(int precision, int64_t rows, int cols);
int nerf_amd_relu_mask_bias(void* delta, const void* act, int precision, int64_t rows, int cols, float* col_sum, void* stream);

/* nerf_amd_train_dump_to_rows and nerf_amd_relu_mask_bias of ONE layer in one pass: act_out (M, n_features) = the layer's activations
 * row-major, delta (M, n_features, same element type) masked in place by [act > 0], and col_sum = nerf_amd_train_dump_rows_mask_partials()
 * rows of n_features fp32 partial column sums of the masked delta (all rows written; their sum is the bias gradient).
 * n_features = 128 or 256. */
int64_t nerf_amd_train_dump_rows_mask_partials(void);
int nerf_amd_train_dump_rows_mask(const void* dump, int net, int precision, int64_t M, int layer, int n_features, void* act_out, void* delta,
                                  float* col_sum, void* stream);

/* Input operand of the first-layer / skip-layer weight gradients: row m = [x | positional_encoding_L(x) (nerf_helper.py:38-48) | 0 ...]
 * with 3 + 6L columns rounded up to a multiple of 8, bf16 (NERF_AMD_BF16) or fp32 rows.  x (M, >=3) with row stride x_stride floats;
 * normalize != 0 divides x by its norm first (the view direction, mip_model.py:52).  L = 4 or 10. */
int nerf_amd_encode_rows(const float* x, int x_stride, int64_t M, int L, int normalize, int precision, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the two MLPs (what torch.autograd computes for addtional.py:88-96 / mip_model.py:41-60 inside train.py:164-199, and the
 * optimizer step of train.py:117-118,200-218) as hand-written kernels -- no library GEMM:
 *   1. nerf_amd_pack_weights_backward: the TRANSPOSED weights in the kernels' fragment order (re-pack after every optimizer step,
 *      like the forward blob; `weights` in the same order as nerf_amd_pack_weights);
 *   2. nerf_amd_{proposal,mip}_backward_chain: the dgrad chain.  Inputs: the gradient w.r.t. the network output (g_density (M) /
 *      g_rgbo (M,4) together with the forward output rgbo (M,4) for the sigmoid adjoint) and the activation dump of the training
 *      forward; output: the "delta dump" (same size and fragment order as the activation dump: nerf_amd_train_dump_bytes);
 *   3. nerf_amd_{proposal,mip}_weight_grads: delta^T . activations on the matrix cores, written as (out, in) row-major fp32 tensors
 *      in the networks' tensor order (d_weights / d_biases: HOST arrays of DEVICE pointers, every tensor fully overwritten);
 *      workspace: nerf_amd_weight_grads_workspace_bytes bytes of device scratch.  Deterministic (no atomics).
 *   4. nerf_amd_adam_step: torch.optim.Adam (no weight decay, no amsgrad) over a table of tensors; `step` is a DEVICE float holding
 *      the number of steps taken so far (incremented by the call, so that a captured graph replays correctly); grads are multiplied
 *      by grad_scale first (1 = plain; 1/world_size after a summing all-reduce).  lr / betas / eps are doubles like torch's Python
 *      scalars (the bias corrections 1 - beta^step are formed in double, as torch does); a non-NULL lr_dev (one double on the device)
 *      overrides lr when the kernel runs, so that a captured graph follows a learning-rate schedule.
 *      grad_scale multiplies every gradient element once, in fp32, before anything else reads it: both moments are formed from
 *      g * grad_scale (exp_avg_sq from its square), and `grads` itself is not written.  The device step counter is an fp32 incremented
 *      by 1.0f per call (once per call, however many table launches the tensor list takes), so it is exact up to 2^24 steps.
 * Gradients w.r.t. the sample positions are not produced (the reference detaches them for these two networks).
 * ------------------------------------------------------------------------------------------------ */
size_t nerf_amd_packed_backward_bytes(int net, int precision);
int    nerf_amd_pack_weights_backward(int net, int precision, const float* const* weights, int n_tensors, void* packed_bwd, void* stream);
int    nerf_amd_proposal_backward_chain(const void* packed_bwd, int precision, const float* g_density, int64_t M, const void* act_dump,
                                        void* delta_dump, void* stream);
int    nerf_amd_mip_backward_chain(const void* packed_bwd, int precision, const float* g_rgbo, const float* rgbo, int64_t M,
                                   const void* act_dump, void* delta_dump, void* stream);
size_t nerf_amd_weight_grads_workspace_bytes(int net, int precision, int64_t M);
int    nerf_amd_proposal_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, float* const* d_weights,
                                      float* const* d_biases, void* workspace, void* stream);
int    nerf_amd_mip_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, const float* const* weights,
                                 const float* const* biases, float* const* d_weights, float* const* d_biases, void* workspace, void* stream);
/* Ref-NeRF training (ref_model.py:68-143, train.py:176-199).
 *   nerf_amd_ref_forward_train_dump: nerf_amd_ref_forward_train + the activation dump (nerf_amd_train_dump_bytes(NERF_AMD_NET_REF, ..))
 *     and aux (M,16) fp32 = the pre-activation head values the backward's element-wise stage needs.
 *   nerf_amd_density_grad: RefNeRF.get_grad's gradient (ref_model.py:119-125 before the normalisation) -- d density / d position of
 *     every sample, times scale[m * scale_stride] when `scale` is given -- for the proposal network (train.py:165-168) or Ref-NeRF's
 *     spatial network (train.py:178): a dgrad-only chain from the density row through the hidden layers (ReLU masks from the dump)
 *     to the encoded position, then the positional encoding's derivative.  x (M, x_stride >= 3) = the sample positions.
 *   nerf_amd_ref_backward: every parameter gradient.  g_out (M, g_stride >= 7) = the gradient w.r.t. [rgb 3 | raw density 1 |
 *     predicted normal 3]; dirs = the view directions the forward saw; ide_table = the (9,19) table given to nerf_amd_pack_weights.
 *     d_weights / d_biases: 20 tensors each -- 0..7 spa_block1.{0,2,4,6}, spa_block2.{0,2,4,6}; 8 bottle_neck; 9 norm_col_tint_head;
 *     10 rho_tau_head; 11..18 dir_block1.{0,2,4,6}, dir_block2.{0,2,4,6}; 19 spec_rgb_head.0 -- (out, in) row-major, fully overwritten.
 *   packed_bwd: nerf_amd_pack_weights_backward(NERF_AMD_NET_REF, ...) with the 20 tensors of nerf_amd_pack_weights. */
int    nerf_amd_ref_forward_train_dump(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, const float* bn_noise,
                                       float* rgbo, float* normal, void* dump, float* aux, void* stream);
/* (ABI 122) The same with the bottle-neck perturbation (ref_model.py:84-85, `spa_info_b + torch.normal(0, w, shape)`) drawn INSIDE the
 * kernel: N(0, noise_std) deviates from Philox4x32-10 + Box-Muller keyed by (noise_seed -- or *noise_seed_dev, read at run time so that a
 * captured hipGraph replays fresh noise --, sample index): no (M, 128) noise tensor is written and read back (1.6 GB and one launch per
 * 2^14-ray step).  nerf_amd_philox_normal materialises exactly those deviates as out (M, 128) for samples sample_offset .. + M - 1
 * (nerf_amd_ref_forward_train_dump with that tensor gives bit-identical outputs). */
int    nerf_amd_ref_forward_train_dump_rng(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, uint64_t noise_seed,
                                           const uint64_t* noise_seed_dev, float noise_std, float* rgbo, float* normal, void* dump, float* aux,
                                           void* stream);
int    nerf_amd_philox_normal(float* out, int64_t M, uint64_t rng_seed, const uint64_t* seed_dev, float std, int64_t sample_offset, void* stream);
/* NERF_AMD_CONTRACTED OR-ed into `net` of nerf_amd_density_grad (round 5): the training forward fetched its samples with
 * nerf_amd_samples.contract = 1 -- x are the UNcontracted positions; the encoding's derivative is taken at contract(x) and pulled back
 * through the contraction's Jacobian, so the result is still d density / d x. */
#define NERF_AMD_CONTRACTED 0x100
size_t nerf_amd_density_grad_workspace_bytes(int net, int precision, int64_t M);
int    nerf_amd_density_grad(int net, const void* packed_bwd, int precision, int64_t M, const void* act_dump, const float* x, int x_stride,
                             const float* scale, int scale_stride, float* grad, void* workspace, void* stream);
size_t nerf_amd_ref_backward_workspace_bytes(int precision, int64_t M);
int    nerf_amd_ref_backward(const void* packed_bwd, int precision, int ref_flags, int64_t M, const void* act_dump, const float* aux,
                             const float* dirs, int dir_stride, const float* g_out, int g_stride, const float* ide_table,
                             float* const* d_weights, float* const* d_biases, void* workspace, void* stream);
int    nerf_amd_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                          const int64_t* numel, int n_tensors, float* step, double lr, const double* lr_dev, double beta1, double beta2,
                          double eps, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Backward of the sampling / compositing rows (what torch.autograd computes for train.py:169-199).
 * One wavefront per ray; S <= 1024 (4, 8 or 16 register chunks of 64 samples, picked by S).  Depths and directions are not differentiated (the reference detaches them too).
 * ------------------------------------------------------------------------------------------------ */
/* d(get_weights)/d(density) (addtional.py:100-107, nerf_base.py:80-86): d_weights (N,S) -> d_sigma (N,S). */
int nerf_amd_sigma_to_weights_backward(const float* sigma, const float* z, const float* dirs, int64_t N, int S, int act,
                                       const float* d_weights, float* d_sigma, void* stream);
/* d(NeRF.render)/d(rgbo) (nerf_base.py:91-113): d_rgb (N,3), optional d_weights (N,S) and d_depth (N) -> d_rgbo (N,S,4);
 * same flags / act / sigma_shift / near / far as nerf_amd_composite. */
int nerf_amd_composite_backward(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S,
                                int flags, int act, float sigma_shift, float near, float far, const float* d_rgb,
                                const float* d_weights, const float* d_depth, float* d_rgbo, void* stream);
/* d(maxBlurFilter)/d(weights) (mip_methods.py:61-66); ties of torch.maximum split the gradient in halves. */
int nerf_amd_max_blur_backward(const float* weights, const float* d_out, int64_t N, int S, float* d_weights, void* stream);
/* d(getBounds)/d(w_prop) (addtional.py:14-18): d_bounds (N,K-1) -> d_w_prop (N,C). */
int nerf_amd_get_bounds_backward(const int64_t* below, const float* d_bounds, int64_t N, int C, int K, float* d_w_prop, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The whole tile body of render_image (procedures.py:64-85, non-Ref) for N rays in four launches:
 *   proposal MLP (stratified z fused) -> resample -> fine MLP (length2pts fused) -> composite.
 * rays: (N,6) device, or NULL to generate them in-kernel from `camera` (mode 2 of nerf_amd_samples;
 * only H, W, fx, fy, pose are read; ray n = row*W + col, n in [ray_offset, ray_offset+N)).
 * z_base (64) = linspace(near, far, 64) (procedures.py:52; an input so that it is bit-identical to the
 * caller's torch.linspace), u_strat (N,64), u_inv (N, n_fine+1) -- or both NULL: every uniform is then drawn inside the kernels
 * (Philox4x32-10, camera->rng_seed / camera->rng_ray_offset; `camera` may accompany explicit rays just to carry them; n_fine <= 255).
 * Outputs rgb (N,3), depth (N) or NULL, weights (N,n_fine) or NULL.
 * workspace: nerf_amd_render_workspace_bytes(N, n_fine) bytes of device scratch.
 * ------------------------------------------------------------------------------------------------ */
/* (With camera != NULL and camera->ipe != 0 -- the descriptor may accompany explicit rays just to carry flags -- the FINE pass uses
 * the integrated positional encoding of the frusta between consecutive fine depths, radius camera->ipe_radius; `rays` must be given.
 * The direction norm of mip_methods.py:31 is taken over the N rays of this call, or -- camera->ipe_dir_norm != NULL -- read from that
 * device scalar: a caller rendering a SHARD of a ray list passes the norm of the whole list (nerf_amd_dirs_norm), so that the shards of an
 * image encode exactly like the single call over all of its rays.) */
size_t nerf_amd_render_workspace_bytes(int64_t N, int n_fine);
int    nerf_amd_render_rays(const void* packed_prop, const void* packed_mip, int precision,
                            const float* rays, const nerf_amd_samples* camera, int64_t ray_offset,
                            const float* z_base, const float* u_strat, const float* u_inv, int64_t N, int n_fine,
                            float near, float far, int white_bkg,
                            float* rgb, float* depth, float* weights, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Disparity ray spacing for unbounded scenes (Mip-NeRF 360, Barron et al. 2022, section 3 and eq. 11-13 with g(x) = 1/x).  Not in the
 * reference: like the contraction this is the build's own definition, parity unpinned.  Samples are drawn and
 * resampled in the normalised distance s in [0, 1], which is uniform in disparity; networks, weights and compositing see metric depths.
 *   constants  gn = fp32(1/near), gf = fp32(1/far): each computed in double and rounded once by the entry point; 0 < near < far
 *   warp       W(s)    = 1 / ((1 - sb) gn + sb gf),   sb = clamp(s, 0, 1)
 *   inverse    W^-1(z) = (1/zb - gn) / (gf - gn),     zb = clamp(z, near, far)
 *              every operation one fp32 rounding in exactly this order (no FMA), IEEE division
 *   coarse     s_j = (float)j r + u r, r = fp32(1/C), j = 0..C-1 (the training sampler's expression at near = 0, far = 1; the reference
 *              render's jitter quirk (far - near)/sample_num is NOT carried into s: it would push s past 1, the warp's pole side)
 *   resample   bins = mid-points of s_c, pdf = maxBlur(get_weights(density, W(s_c) |d|))[1:-1] + 1e-5, K sorted draws s_f, z_f = W(s_f);
 *              `below` keeps its meaning (nerf_amd_get_bounds is untouched)
 *   depth      W^-1(sum w z |d|) in [0, 1]
 * `spacing` must be NERF_AMD_SPACING_DISPARITY in every entry point below (anything else: NERF_AMD_EINVAL); linear spacing is what all
 * the other entry points do and never reaches this code.
 * ------------------------------------------------------------------------------------------------ */
#define NERF_AMD_SPACING_LINEAR    0
#define NERF_AMD_SPACING_DISPARITY 1
/* Elementwise over in (N,S), N >= 0, S >= 1: out = W(in), or with inverse != 0 out = W^-1(in).  pts (N,S,3) = o + out d from rays (N,6)
 * with the arithmetic of nerf_amd_stratified_points, or NULL to skip (forward only). */
int nerf_amd_warp_depths(const float* in, const float* rays, int64_t N, int S, int inverse, int spacing, float near, float far,
                         float* out, float* pts, void* stream);
/* The coarse draw: u (N,C) -- or NULL: word 0 of the 'RS' Philox block of global ray n + rng_ray_offset, the stratified stream of
 * nerf_amd_samples -- -> s_c (N,C), z_c (N,C) = W(s_c), pts (N,C,3) = o + z_c d or NULL.  3 <= C <= 256 (C <= 64 with u == NULL: the
 * stream's 64 slots). */
int nerf_amd_warped_stratified(const float* rays, const float* u, int64_t N, int C, uint64_t rng_seed, int64_t rng_ray_offset, int spacing,
                               float near, float far, float* s_c, float* z_c, float* pts, void* stream);
/* nerf_amd_resample's twin (one wavefront per ray, the same device functions for weights and inverse sampling): density (N,C) and
 * s_c (N,C) -> z_fine (N,K) = W(s_fine), optional s_fine (N,K) sorted, below (N,K) int64, w_prop (N,C).  u_inv (N,K), or NULL: words
 * 1..3 of the 'RS' blocks as in nerf_amd_resample.  3 <= C <= 256, 1 <= K <= 1024 and 4 (5 C + 4 K + 1280) floats of LDS <= 64 KiB. */
int nerf_amd_warped_resample(const float* density, const float* s_c, const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C,
                             int K, int softplus_density, float blur_alpha, int spacing, float near, float far, uint64_t rng_seed,
                             int64_t rng_ray_offset, float* z_fine, float* s_fine, int64_t* below, float* w_prop, void* stream);
/* nerf_amd_render_rays under disparity spacing (non-Ref), six launches: coarse draw -> proposal MLP (explicit z_c) -> warped resample
 * -> fine MLP (explicit z_fine; contract / ipe carried by `camera` as in nerf_amd_render_rays) -> composite -> depth = W^-1(sum w z |d|).
 * Arguments as nerf_amd_render_rays without z_base; every argument is validated before the first launch.  n_fine <= 623: the LDS bound of
 * nerf_amd_warped_resample at C = 64, K = n_fine + 1. */
size_t nerf_amd_render_warped_workspace_bytes(int64_t N, int n_fine);
int    nerf_amd_render_rays_warped(const void* packed_prop, const void* packed_mip, int precision, const float* rays,
                                   const nerf_amd_samples* camera, int64_t ray_offset, const float* u_strat, const float* u_inv, int64_t N,
                                   int n_fine, int spacing, float near, float far, int white_bkg, float* rgb, float* depth, float* weights,
                                   void* workspace, void* stream);

/* Mip-NeRF 360's TWO proposal rounds behind one entry point (non-Ref; in-kernel Philox uniforms only: `camera` is required and carries
 * rng_seed, rng_ray_offset, contract and the ipe fields as in the two entry points above).  `spacing`: NERF_AMD_SPACING_LINEAR or
 * NERF_AMD_SPACING_DISPARITY; z_base (64 floats) is read under linear spacing only.
 *   linear:    [ray generation] -> [IPE direction norm] -> proposal MLP (stratified draw fused) -> resample to prop_pnum sorted depths z_mid
 *              -> proposal MLP at z_mid -> resample to n_fine + 1 depths -> fine MLP -> composite
 *   disparity: coarse draw in s -> proposal MLP -> warped resample to s_mid, z_mid = W(s_mid) -> proposal MLP at z_mid -> warped resample
 *              from s_mid -> fine MLP -> composite (near = 0, far = 1) -> depth = W^-1(sum w z |d|)
 * Uniforms: the stratified stream as in nerf_amd_render_rays; the ray's inverse-CDF stream (words 1..3 of its 'RS' blocks, column k =
 * nerf_amd_philox_stream's column k) has prop_pnum + n_fine + 1 columns: columns [0, prop_pnum) feed the first resampling, columns
 * [prop_pnum, prop_pnum + n_fine + 1) the second -- both keyed by the global ray index n + rng_ray_offset, so any split of a ray list
 * reproduces the whole bit for bit.  The image equals the same chain written with the single-stage entry points on those columns.
 * Limits (NERF_AMD_EINVAL before the first launch): 3 <= prop_pnum <= 256, 1 <= n_fine <= 1023, and both resampling launches within
 * 64 KiB of LDS: linear 4 (5 * 64 + 2 prop_pnum + 1280) and 4 (5 prop_pnum + 3 (n_fine + 1) + 1280) floats, disparity
 * 4 (5 * 64 + 4 prop_pnum + 1280) and 4 (5 prop_pnum + 4 (n_fine + 1) + 1280); the 128-wide fine layout takes no IPE.
 * Workspace (nerf_amd_render_rounds_workspace_bytes; 0 for arguments outside the limits), every part rounded up to 256 bytes:
 *   density (N,64) [| s_c (N,64) | z_c (N,64), disparity] | density2 (N,prop_pnum) | z_mid (N,prop_pnum) [| s_mid (N,prop_pnum), disparity]
 *   | z_fine (N, n_fine+1) | rgbo (N, n_fine, 4) [| raw depth (N), disparity] | rays (N,6) | 512 bytes (scalar slot, alignment slack)
 * No allocation, no synchronisation: capturable like the other render entry points. */
size_t nerf_amd_render_rounds_workspace_bytes(int64_t N, int n_fine, int prop_pnum, int spacing);
int    nerf_amd_render_rays_rounds(const void* packed_prop, const void* packed_mip, int precision, const float* rays,
                                   const nerf_amd_samples* camera, int64_t ray_offset, const float* z_base, int64_t N, int n_fine,
                                   int prop_pnum, int spacing, float near, float far, int white_bkg, float* rgb, float* depth,
                                   float* weights, void* workspace, void* stream);

/* The same tile body for a Ref-NeRF fine network (procedures.py:64-85 with the is_ref_model branch, lines 71-74): proposal pass,
 * resampling, the n_fine+1 fine and 64 coarse depths merged (the last one dropped), Ref-NeRF MLP on the n_fine+64 samples,
 * compositing with sigma -> softplus(sigma + 0.5).  normal_img (N) and cam_dir (3 floats on the device: render_pose[:, -2]) are
 * both given or both NULL (procedures.py:79-81).  Six launches.  Workspace: nerf_amd_render_ref_workspace_bytes(N, n_fine). */
size_t nerf_amd_render_ref_workspace_bytes(int64_t N, int n_fine);
int    nerf_amd_render_rays_ref(const void* packed_prop, const void* packed_ref, int precision, int ref_flags, const float* rays,
                                const nerf_amd_samples* camera, int64_t ray_offset, const float* z_base, const float* u_strat,
                                const float* u_inv, int64_t N, int n_fine, float near, float far, int white_bkg, const float* cam_dir,
                                float* rgb, float* depth, float* normal_img, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (added after ABI 125; additive) Quantile (median) ray-termination depth and accumulated opacity of composited rays: what Mip-NeRF 360
 * and the viewers built on it show instead of the expected depth sum w t, which a little weight far out drags through empty space.  Not
 * in the reference; the build's own definition, restated in fp64 by tests/depth_stats_ref.py.  Per ray:
 *   weights w_0 .. w_{S-1} (fp32, >= 0); depths z_0 .. z_{E-1}, E = S + 1 (`closed` != 0: the row also holds the edge that closes the last
 *   interval) or E = S (open); direction d.  t_s = z_s |d| with mul_norm (one fp32 product, |d| as in nerf_amd_composite), else t_s = z_s.
 *   cumulative mass in fp64: C_0 = 0, C_{s+1} = C_s + (double)w_s;   opacity = (float)C_S
 *   for each quantile q (fp32, 0 < q < 1, at most NERF_AMD_DEPTH_QUANTILES_MAX per call) -- the mass is ABSOLUTE, not renormalised
 *   (multinerf's weighted_percentile): k = the smallest s with C_{s+1} >= q;
 *       no such s (the ray never accumulates q):  D_q = t_{E-1}      (the far edge)
 *       k = S - 1 of an open row:                 D_q = t_{S-1}
 *       otherwise                                 D_q = t_k + ((q - C_k) / w_k) (t_{k+1} - t_k)    in fp64, rounded once to fp32
 *   depth_q = (D_q - near) / (far - near) in fp32, as nerf_amd_composite normalises its depth.
 * D_q is continuous in the weights except where the crossing sits exactly on an edge next to a zero-weight interval.
 * weights (N,S); z rows of z_stride >= E floats; dirs rows of dirs_stride floats (read with mul_norm only); quantiles: HOST array;
 * opacity (N) or NULL; depth_q (N, n_quantiles) or NULL.  Refused before the launch: NULL inputs, N < 0, S < 1, n_quantiles outside
 * 0..NERF_AMD_DEPTH_QUANTILES_MAX, a q outside (0, 1) or NaN, z_stride < E.  N == 0 is fine.  One launch, one wavefront per ray, any S;
 * no workspace, no atomics, no host state: deterministic and capturable.
 * ------------------------------------------------------------------------------------------------ */
#define NERF_AMD_DEPTH_QUANTILES_MAX 4
int nerf_amd_ray_depth_stats(const float* weights, const float* z, int z_stride, int closed, const float* dirs, int dirs_stride, int64_t N,
                             int S, int mul_norm, const float* quantiles, int n_quantiles, float near, float far, float* opacity,
                             float* depth_q, void* stream);

/* (added after ABI 125; additive) The four render entry points above behind ONE request: the same pipeline, the same launches, plus
 * optional outputs they have no argument for.  `size` = sizeof(nerf_amd_render_request) of the caller's header (the first layout's 200 bytes --
 * everything up to fine_depths -- are accepted too, with the later fields off; anything smaller is refused); zero-fill the struct, then
 * set what the call uses.
 *   which entry point:  ref != 0 -> nerf_amd_render_rays_ref;  else prop_pnum != 0 -> nerf_amd_render_rays_rounds (in-kernel uniforms only);
 *                       else spacing == NERF_AMD_SPACING_DISPARITY -> nerf_amd_render_rays_warped;  else nerf_amd_render_rays.
 *   Every field means what the argument of that name means there (`normal_img` / `cam_dir` / `ref_flags` are read for Ref-NeRF only;
 *   `weights` is (N, n_fine) for MipNeRF and -- through this entry point alone -- (N, n_fine + 64) for Ref-NeRF; with two rounds u_strat and
 *   u_inv must be NULL).  With opacity, depth_q and fine_depths NULL the call IS that entry point: same checks, same launches, same bits,
 *   and nerf_amd_render_request_workspace_bytes equals its workspace query.  (Inside the library the four fill such a request themselves and
 *   go this way; the Python package calls nerf_amd_render alone, and the four argument-list symbols are kept for C callers.)
 *   opacity (N), depth_q (N, n_quantiles) with quantiles[0 .. n_quantiles): nerf_amd_ray_depth_stats of the weights and depth row the fine
 *   pass composited (mul_norm; closed rows of n_fine + 1 depths on the MipNeRF routes, open rows of n_fine + 64 for Ref-NeRF; near, far of
 *   the request -- under disparity spacing near = 0, far = 1 followed by W^-1 like `depth`, so depth_q lives in the same [0, 1] s-scale).
 *   fine_depths (N, E): a copy of that depth row, E = n_fine + 1 (MipNeRF) or n_fine + 64 (Ref-NeRF).
 *   They append to the entry point's launches: the stats launch [-> the un-warp] [-> one device-to-device copy].  The kernel reads the
 *   weights the compositing kernel wrote: `weights` when given, else a part appended BEHIND the entry point's workspace (as is the raw
 *   depth_q under disparity spacing) -- nerf_amd_render_request_workspace_bytes grows by those parts, the existing layout does not move.
 * ------------------------------------------------------------------------------------------------ */
typedef struct nerf_amd_render_request {
    size_t size;                       /* sizeof(nerf_amd_render_request) */
    const void* packed_prop;
    const void* packed_fine;           /* MipNeRF blob, or the Ref-NeRF blob with ref != 0 */
    int32_t precision;                 /* NERF_AMD_F32 / NERF_AMD_BF16, layout flags OR-ed in */
    int32_t ref;                       /* != 0: Ref-NeRF fine network */
    int32_t ref_flags;                 /* NERF_AMD_REF_SRGB */
    int32_t white_bkg;
    const float* rays;                 /* (N,6), or NULL with `camera` */
    const nerf_amd_samples* camera;
    int64_t ray_offset;
    const float* z_base;               /* (64), linear spacing */
    const float* u_strat;              /* (N,64) and (N, n_fine+1), or both NULL: in-kernel uniforms */
    const float* u_inv;
    int64_t N;
    int32_t n_fine;
    int32_t prop_pnum;                 /* 0: one proposal round */
    int32_t spacing;                   /* NERF_AMD_SPACING_LINEAR / NERF_AMD_SPACING_DISPARITY */
    float near, far;
    int32_t n_quantiles;               /* 0 .. NERF_AMD_DEPTH_QUANTILES_MAX */
    float quantiles[NERF_AMD_DEPTH_QUANTILES_MAX];
    const float* cam_dir;              /* (3) device, with normal_img */
    float* rgb;                        /* (N,3) */
    float* depth;                      /* (N) or NULL */
    float* weights;                    /* (N, n_fine), Ref-NeRF (N, n_fine + 64), or NULL */
    float* normal_img;                 /* (N) or NULL (Ref-NeRF) */
    float* opacity;                    /* (N) or NULL */
    float* depth_q;                    /* (N, n_quantiles) or NULL */
    float* fine_depths;                /* (N, E) or NULL */
    /* -- end of the first layout (200 bytes); a `size` of exactly that is accepted and leaves everything below off -- */
    double skip_min_optical_depth;     /* D_min of the empty-ray skip (below); <= 0: off */
    int32_t* row_of_ray;               /* (N) device output or NULL: the compact row of each ray, -1 = skipped (skip on only) */
    int64_t* n_alive;                  /* HOST output or NULL: the number of rays the fine network ran on (skip on only) */
} nerf_amd_render_request;
size_t nerf_amd_render_request_workspace_bytes(const nerf_amd_render_request* request);
int    nerf_amd_render(const nerf_amd_render_request* request, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * (added after ABI 125; additive) Skip the fine pass for rays the proposal histogram leaves empty.  Opt-in; not in the reference: the
 * build's own definition, restated in fp64 by tests/skip_empty_ref.py.  Per ray, with the raw proposal densities sigma_0 .. sigma_{C-1}
 * (fp32), their ascending metric depths z_0 .. z_{C-1} (fp32) and the direction d, everything in fp64 from those fp32 values:
 *
 *     D     = |d| * sum_{s < C-1} max(sigma_s, 0) * (z_{s+1} - z_s)  +  max(sigma_{C-1}, 0) * 1e10        |d| = sqrt(dx^2 + dy^2 + dz^2)
 *     alive = !(D < D_min)
 *
 * the optical depth of ProposalNetwork.get_weights (addtional.py:103-104: the last delta is 1e10 and is not scaled by |d|).  max keeps a
 * NaN, so a NaN density keeps the ray alive and it renders as the dense path would; any positive density at the far sample keeps it alive
 * too (it makes the ray opaque in the reference's own weights).  The user-facing threshold is an opacity tau in (0, 1):
 * D_min = -log1p(-tau), computed by the caller in double.  fp64 summation order is not specified: a ray with |D - D_min| <= 1e-9 max(D,
 * D_min) may fall either way.
 *
 * nerf_amd_ray_alive: density (N,C) contiguous, z rows of z_stride >= C floats, dirs rows of dirs_stride >= 3 floats ->
 *   row_of_ray (N) int32: the rank of ray n among the alive rays, -1 for a dead one;  ray_of_row (>= N' entries are written, N' <= N)
 *   int64: the inverse list, ascending;  count_dev: one int64 ON THE DEVICE = N'.  Alive rays keep their order: the tables are a pure
 *   function of the inputs (ballot + popcount per wave, a two-level scan of 256-ray tiles; no atomics).  Four launches; workspace of
 *   nerf_amd_ray_alive_workspace_bytes(N) bytes.  Refused before the first launch: NULL arguments (N > 0), N < 0 or N >= 2^31, C < 2,
 *   z_stride < C, dirs_stride < 3, a NaN min_optical_depth.  N == 0 is fine (*count_dev = 0).
 * nerf_amd_gather_rows: dst (n_rows, cols) contiguous = rows ray_of_row[0 .. n_rows) of src (row stride src_stride >= cols floats).
 *
 * In nerf_amd_render (skip_min_optical_depth > 0) the stage runs after the last resampling (Ref-NeRF: after the depth merge), on the
 * histogram the fine depths were drawn from -- one round: the proposal densities at the 64 coarse depths (linear spacing: the resampling
 * kernel also stores the depths it drew, through the z_coarse output it has for Ref-NeRF; disparity: the metric row z_c); two rounds: the
 * second pass's densities at z_mid; Ref-NeRF: the densities at z_coarse -- then: N' is read back to the host (one hipMemcpyAsync + one
 * hipStreamSynchronize), the alive rays' ray records and fine depth rows are gathered into compact tables, the fine network runs on N'
 * rays (none is launched for N' = 0) and writes compact rows, and compositing reads ray n's row at row_of_ray[n], an ALL-ZERO row for a
 * dead ray; depths, weights and every output stay (N, ...) and are indexed by the ray.  So every output equals the dense call's with the
 * fine network's rows of the dead rays replaced by zeros, bit for bit: an alive ray is the dense ray; a dead MipNeRF ray is
 * nerf_amd_composite of zero density on its own depth row -- background colour, zero weights, opacity 0, the far edge as quantile depth;
 * with D_min so small that every ray is alive the call is the dense call.  (Ref-NeRF composites softplus(sigma + 0.5): a zero row is
 * NOT zero density there -- a dead Ref-NeRF ray is the composite of that constant density with zero colour.)  This is an approximation
 * of the image: its error is the fine opacity of the rays the proposal network calls empty.  The integrated PE keeps the direction norm
 * of the whole ray list.  The call reads a count on the host: it is NOT capturable and is refused with NERF_AMD_EUNSUPPORTED on a
 * capturing stream.  The skip's workspace parts (tables, flags, the compact ray and depth tables, the stored coarse depths) are appended
 * behind everything else: only nerf_amd_render_request_workspace_bytes grows; the four argument-list entry points cannot carry the skip.
 * ------------------------------------------------------------------------------------------------ */
size_t nerf_amd_ray_alive_workspace_bytes(int64_t N);
int    nerf_amd_ray_alive(const float* density, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int C,
                          double min_optical_depth, int32_t* row_of_ray, int64_t* ray_of_row, int64_t* count_dev, void* workspace,
                          void* stream);
int    nerf_amd_gather_rows(const float* src, int64_t src_stride, const int64_t* ray_of_row, int64_t n_rows, int cols, float* dst,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generic-shape layer product (ABI 119): the path of networks LARGER than the shapes the fused MLP kernels are compiled for -- hidden
 * widths above 256 (`--nerf_net_width` / `--prop_net_width`, procedures.py:176-177), more than 10 encoding octaves (mip_model.py:15-18,
 * addtional.py:61).  Such a network is evaluated layer by layer (nerf_helper.py:28-36 makeMLP = nn.Linear + activation) with fp32
 * row-major activations in HBM, forward and backward, by ONE hand-written MFMA GEMM with explicit element strides:
 *
 *     C[i, j] = act( sum_{p < P} A[i*a_si + p*a_sp] * B[p*b_sp + j*b_sj] + bias[j] ) * [mask[i*ldm + j] > 0]        i < M, j < N
 *
 *   forward  y = act(x W^T + b): A = x, B(p, j) = W[j, p];   input gradient  dx = (dy W) . [x > 0]: A = dy, B = W, mask = x;
 *   weight gradient  dW = dy^T x: A(i, p) = dy[p, i], B = x (db: B = a column of ones) -- a long contraction over the samples is split
 *   over workgroups, partial sums in `workspace` (nerf_amd_gemm_workspace_bytes bytes; may be NULL when that is 0), added in a fixed
 *   order: deterministic, no atomics.
 * Of each operand's two strides one must be 1.  C row-major, row stride ldc.  bias (N) or NULL; act 0 none / 1 ReLU / 2 sigmoid; mask or NULL.
 * precision: NERF_AMD_F32 = v_mfma_f32_32x32x2_f32 on the fp32 operands; NERF_AMD_BF16 = operands rounded to bf16 (RNE), fp32 accumulation.
 * All matrices fp32 on the device.  Every compiled shape keeps its fused kernel; this is the compatibility path of the shape arguments. */
size_t nerf_amd_gemm_workspace_bytes(int64_t M, int64_t N, int64_t P);
int    nerf_amd_gemm(int precision, int64_t M, int64_t N, int64_t P, const float* A, int64_t a_si, int64_t a_sp,
                     const float* B, int64_t b_sp, int64_t b_sj, float* C, int64_t ldc, const float* bias, int act,
                     const float* mask, int64_t ldm, void* workspace, void* stream);
/* out[m, c] = g[m, c] * y[m, c] * (1 - y[m, c]), c < cols: the adjoint of y = sigmoid(.) (rgb_layer.2, mip_model.py:35); row strides in floats */
int    nerf_amd_sigmoid_backward(const float* g, int64_t g_stride, const float* y, int64_t y_stride, int64_t M, int cols,
                                 float* out, int64_t out_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Generic-shape Ref-NeRF (ABI 120): a RefNeRF the fused kernel is not compiled for -- hidden width above 256, more than 10 position
 * octaves, `--ide_level 5` (procedures.py:211; 36 spherical-harmonic terms) -- runs layer by layer on nerf_amd_gemm; these are the
 * element-wise stages between its layer products (ref_model.py:78-105), forward and adjoint.  One row per sample, fp32, explicit row
 * strides in floats (column ranges of a concatenated buffer are views).  `heads` (M, >= 11) = the raw outputs of
 * cat(norm_col_tint_head, rho_tau_head):  [normal 0-2 | diffuse 3-5 | tint 6-8 | roughness 9 | density 10].
 *
 *   nerf_amd_ref_dir_inputs            ref_model.py:80-92: roughness = softplus(rho - 1), n = -n / (|n| + 1e-7), w_r = d - 2 (d.n) n, the
 *                                      integrated directional encoding of ref_func.py:76-108 at `ide_level` 1..5 (T = 2^level - 1 + level
 *                                      terms; `ide_table` = its (2^(level-1) + 1, T) coefficient matrix, ref_func.py:60-74) and n.d
 *                                      -> out (M, >= 2T+1) = [IDE real T | IDE imag T | n.d], normal (M,3) contiguous
 *   nerf_amd_ref_dir_inputs_backward   d_out (M, >= 2T+1), g_normal (M, >= 3) -> d_heads columns 0-2 (normal) and 9 (roughness)
 *   nerf_amd_ref_combine               ref_model.py:98-105: rgb = spec * sigmoid(tint) + sigmoid(diffuse) (NERF_AMD_REF_SRGB: linear_to_srgb(
 *                                      spec * sigmoid(tint) + sigmoid(diffuse - log 3))), `spec` (M, >= 3) = sigmoid(spec_rgb_head);
 *                                      rgbo (M,4) contiguous = [rgb | raw density]
 *   nerf_amd_ref_combine_backward      g_rgbo (M, >= 4) -> d_spec (M, >= 3) w.r.t. spec_rgb_head's PRE-activation, d_heads columns 3-8, 10
 *   nerf_amd_positional_encoding_backward   d_x (M,3) = (d [x | sin 2^f x | cos 2^f x] / d x)^T d_enc, f < L (nerf_helper.py:38-48 layout behind
 *                                      the raw position when cat_origin): RefNeRF.get_grad's last step (ref_model.py:119-125)
 *   nerf_amd_add_rows                  dst[m, c] += src[m, c], c < cols
 */
int nerf_amd_ref_dir_inputs(const float* heads, int64_t heads_stride, const float* dirs, int64_t dirs_stride, int64_t M, int ide_level,
                            const float* ide_table, float* out, int64_t out_stride, float* normal, void* stream);
int nerf_amd_ref_dir_inputs_backward(const float* heads, int64_t heads_stride, const float* dirs, int64_t dirs_stride, int64_t M, int ide_level,
                                     const float* ide_table, const float* d_out, int64_t d_out_stride, const float* g_normal,
                                     int64_t g_normal_stride, float* d_heads, int64_t d_heads_stride, void* stream);
int nerf_amd_ref_combine(const float* heads, int64_t heads_stride, const float* spec, int64_t spec_stride, int64_t M, int ref_flags,
                         float* rgbo, void* stream);
int nerf_amd_ref_combine_backward(const float* g_rgbo, int64_t g_stride, const float* heads, int64_t heads_stride, const float* spec,
                                  int64_t spec_stride, int64_t M, int ref_flags, float* d_spec, int64_t d_spec_stride, float* d_heads,
                                  int64_t d_heads_stride, void* stream);
int nerf_amd_positional_encoding_backward(const float* d_enc, int64_t d_enc_stride, const float* x, int64_t x_stride, int64_t M, int L,
                                          int cat_origin, float* d_x, void* stream);
int nerf_amd_add_rows(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, int64_t M, int cols, void* stream);
/* (ABI 123) Mip-NeRF 360 scene contraction as a stage of the layer-by-layer route (the fused kernels apply it in their sample fetch:
 * nerf_amd_samples.contract): g == NULL -> out (M,3) = contract(x); g (M, g_stride >= 3) = a gradient w.r.t. contract(x) -> out (M,3) = its
 * pull-back through the contraction's Jacobian (what RefNeRF.get_grad needs, ref_model.py:119-125).  Not in the reference (BASELINE
 * configs[4]); the definition is oracle.contract. */
int nerf_amd_contract_positions(const float* x, int64_t x_stride, int64_t M, const float* g, int64_t g_stride, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layer products on bf16 rows (ABI 124): the INFERENCE route of the networks above under bf16 precision (forward only; nerf_amd_gemm
 * stays the fp32 parity mode and the backward).  One nn.Linear (+ activation) of mip_model.py:41-60 / addtional.py:88-96 /
 * ref_model.py:68-106:
 *
 *     C[m, n] = act( sum_k X[m, k] * W[n, k] + bias[n] ),   m < M, n < N, k < K
 *
 *   X     bf16 rows, row stride ldx ELEMENTS (a multiple of 8), 16-byte aligned; elements K .. roundup(K, 8) - 1 of a row must be finite
 *         (they meet packed zero weights): the padding nerf_amd_rows_to_bf16 writes, or the neighbouring columns of a wider buffer
 *   W     the layer's weight (N, K) as bf16 rows, zero-padded to (n_pad, ldw): n_pad a multiple of 256 >= N, ldw a multiple of 64 >= K
 *         (nerf_amd_rows_to_bf16 with rows = n_pad, fill = ldw packs an fp32 nn.Linear.weight)
 *   bias  n_pad floats (zeros beyond N), 16-byte aligned
 *   C     out_bf16 != 0: bf16 rows for the next layer (N % 4 == 0, ldc % 4 == 0, 8-byte aligned); else fp32 rows (any N / ldc): the
 *         heads, and the inputs of the element-wise stages
 *   act   0 none / 1 ReLU / 2 sigmoid
 * 256 x 256 outputs per workgroup, both operands global -> LDS by DMA through a 4-slot ring, v_mfma_f32_32x32x16_bf16, fp32 accumulation:
 * the values nerf_amd_gemm(NERF_AMD_BF16) computes (it rounds the same operands on their way into LDS), at 3x its rate. */
int nerf_amd_rows_gemm(int64_t M, int64_t N, int64_t K, const void* X, int64_t ldx, const void* W, int64_t ldw, int64_t n_pad,
                       const float* bias, int act, void* C, int64_t ldc, int out_bf16, void* stream);
/* dst[m, j] = bf16(src[m, j]) (RNE) for m < rows_src, j < cols; 0 for the rest of rows x fill: fp32 rows (row stride src_stride floats)
 * into a column range of bf16 rows (dst = first element of the range, row stride dst_stride elements) with the zero padding above */
int nerf_amd_rows_to_bf16(const float* src, int64_t rows_src, int64_t src_stride, int64_t rows, int cols, int fill, void* dst,
                          int64_t dst_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Image metrics (additive; the ABI number stays): SSIM and MSE of rendered views against their ground truth, per view, on the device.
 *
 *   pred, target   contiguous fp32 (V, C, H, W), V >= 1, C >= 1, H >= 11, W >= 11.  Values are nominally in [0, 1], the dynamic range is
 *                  L = 1; values outside [0, 1] are legal and go through the same formulas.
 *   window         g[i] ~ exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0 .. 10, normalised to sum 1 in fp64 on the host and handed to the kernel as
 *                  11 fp32 constants; the 2-D window is g g^T (separable).
 *   positions      VALID ones only: the map has (H - 10) x (W - 10) entries per (view, channel); no padding of any kind.
 *   per position   with <.> the windowed average:
 *                      mu_x = <x>, mu_y = <y>, s_x^2 = <x^2> - mu_x^2, s_y^2 = <y^2> - mu_y^2, s_xy = <xy> - mu_x mu_y
 *                      C1 = (0.01 L)^2, C2 = (0.03 L)^2
 *                      SSIM = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2))
 *                  No clamp belongs to the definition.  The kernel forms the fp32 moments about 0.5 (of a = x - 0.5, b = y - 0.5; the
 *                  variances do not depend on the offset, mu_x = 0.5 + <a>); tests/image_metrics_ref.py bounds its rounding per position.
 *   ssim_out[v]    fp64: the mean of the map over channels and valid positions
 *   mse_out[v]     fp64: the mean of (x - y)^2 over ALL C H W elements of the view (the difference in fp32, its square and the sums in
 *                  fp64); exactly 0 for identical images.  PSNR = -10 log10(mse) is left to the caller.
 *   ssim_map       optional (NULL: not written): fp32 (V, C, H - 10, W - 10)
 *   workspace      nerf_amd_image_metrics_workspace_bytes(V, C, H, W) bytes, 8-byte aligned, any content: one (SSIM sum, squared-difference
 *                  sum) pair of fp64 per workgroup.  A workgroup walks one segment of one plane's map, NERF_AMD_IMAGE_METRICS_SEGMENT_H rows
 *                  by _TILE_W columns, in tiles of _TILE_H rows.
 * Two launches, no atomics, no host synchronisation, no allocation: the partials are added in a fixed order, so the outputs are a
 * function of the inputs' bits alone, a view's values do not depend on the other views of the call, and the call can be captured into
 * a graph.  V * C * H * W may exceed 2^31; V * C * segments must stay below 2^31.
 * NERF_AMD_EINVAL (with a message): H or W < 11, a non-positive size, a NULL required pointer, too many segments. */
#define NERF_AMD_IMAGE_METRICS_TILE_H 16
#define NERF_AMD_IMAGE_METRICS_TILE_W 64
#define NERF_AMD_IMAGE_METRICS_SEGMENT_H 128
size_t nerf_amd_image_metrics_workspace_bytes(int64_t V, int C, int H, int W);
int nerf_amd_image_metrics(const float* pred, const float* target, int64_t V, int C, int H, int W, double* mse_out, double* ssim_out,
                           float* ssim_map, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Iso-surface extraction (additive; the ABI number stays): a triangle mesh of { f = iso } from a lattice of field values (for a NeRF:
 * the density), by marching tetrahedra on the Kuhn split of every cell into six tetrahedra.  The build's own definition (nothing of the
 * kind is in the reference); tests/mesh_ref.py restates it in fp64 without a case table.
 *
 *   field      contiguous fp32 (nz, ny, nx), x fastest; every dimension >= 2, nx * ny * nz < 2^31.  Lattice point (i, j, k) has the
 *              linear index p = (k ny + j) nx + i and the position origin + spacing * (i, j, k) (component-wise).
 *   inside     a point is inside when f >= iso, on the fp32 values; a NaN is outside.
 *   edges      every point a owns 7 edge slots s = 0..6 with direction d = ((s+1) & 1, ((s+1) >> 1) & 1, ((s+1) >> 2) & 1): the three axis
 *              edges, the three face diagonals and the body diagonal, all towards +.  The edge a -> b = a + d exists if b is in the
 *              lattice and carries a vertex if inside(a) != inside(b).
 *   vertices   numbered in ascending (p, s).  t = (iso - f_a) / (f_b - f_a) in fp32 (two subtractions, one division), a non-finite t
 *              becomes 0.5 (so +-inf entries still give finite positions), else t is clamped to [0, 1]; always measured from the owner a.
 *              position = origin + spacing * (a + t d), per component: fl(a + t) where d is 1, one multiplication, one addition.
 *   normals    optional.  g = the central difference of the field at a and at b, one-sided on the lattice's faces:
 *              (f[hi] - f[lo]) / (spacing (hi - lo)) per axis.  n = -normalize((1 - t) g_a + t g_b); a zero or non-finite vector is
 *              stored as (0, 0, 0).  The normal points from high values to low, like the winding.
 *   cells      named by their lowest corner p (i < nx-1, j < ny-1, k < nz-1).  The six tetrahedra are the axis permutations (a1, a2, a3) in
 *              lexicographic order xyz, xzy, yxz, yzx, zxy, zyx, with corners v0 = the cell's corner, v1 = v0 + e_a1, v2 = v1 + e_a2,
 *              v3 = v2 + e_a3.  Every tetrahedron edge is one of the 7 slot directions from its component-wise lower end, which owns it.
 *   triangles  of one tetrahedron, with I the inside local corners ascending, O the outside ones, E(u, w) the vertex on edge u-w:
 *                  |I| = 1: a = I0, (b, c, d) = O:   (E(a,b), E(a,c), E(a,d))
 *                  |I| = 3: a = O0, (b, c, d) = I:   the same expression
 *                  |I| = 2: (a, b) = I, (c, d) = O:  (E(a,c), E(a,d), E(b,d)) then (E(a,c), E(b,d), E(b,c))
 *   winding    the 2nd and 3rd entry of a triangle are swapped when needed so that, with every crossing placed at the MIDPOINT of its edge,
 *              (p1 - p0) x (p2 - p0) has a positive dot product with (mean of the outside corners - mean of the inside corners): an exact
 *              integer test on lattice coordinates, independent of t and therefore of ties f == iso.  A closed iso-surface comes out
 *              closed and consistently oriented: there are no ambiguous faces.
 *   faces      int32 vertex ids, ordered by ascending (cell p, tetrahedron, triangle).
 *
 * Two calls, with the caller reading the counts in between (the pair is therefore not capturable into a graph):
 *   nerf_amd_mesh_count   classifies every point (one byte: the crossed slots and the inside flag; the later passes do not read the
 *                         field to classify), counts vertices and triangles per tile of 256 points, scans the tiles and stores
 *                         counts_dev[0] = vertices, counts_dev[1] = faces (device, int64).
 *   nerf_amd_mesh_emit    with the SAME field, shape, iso and workspace: stores vertices (V, 3) fp32, normals (V, 3) fp32 unless NULL, and
 *                         faces (F, 3) int32.  Every store is guarded by vertex_capacity / face_capacity (in vertices / faces): with
 *                         capacities below the counts the first entries are written and nothing beyond them.  origin_host and
 *                         spacing_host are three floats each on the host.
 *   workspace             nerf_amd_mesh_workspace_bytes(nx, ny, nz) bytes (0: the shape is refused), about 5 bytes per point: the byte,
 *                         and one int32 per point -- the id of its first vertex; the id of (p, s) is that plus the number of crossed
 *                         slots below s.  Any content on entry to nerf_amd_mesh_count.
 * No atomics: wave scans, popcounts and one scan of the tile counts; the outputs are a function of the inputs' bits alone.
 * NERF_AMD_EINVAL (with a message), before any launch: a NULL pointer (only normals is optional; vertices / faces may be NULL with a zero
 * capacity), a dimension < 2, nx * ny * nz >= 2^31, a non-finite iso or origin, a spacing that is not positive and finite, a capacity that
 * is negative or would let a vertex id or 3 * faces reach 2^31. */
#define NERF_AMD_MESH_SCAN_STEP_TILES 4096 /* tiles of 256 points per step of the one workgroup that scans the tile counts */
size_t nerf_amd_mesh_workspace_bytes(int nx, int ny, int nz);
int nerf_amd_mesh_count(const float* field, int nx, int ny, int nz, float iso, int64_t* counts_dev, void* workspace, void* stream);
int nerf_amd_mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin_host, const float* spacing_host,
                       void* workspace, int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_AMD_H */
