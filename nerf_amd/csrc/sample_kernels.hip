// Sampling / compositing kernels: one 64-lane wavefront per
// ray, samples across lanes, wave-level prefix scans for transmittance and CDF.  All HBM-bound.
//
// Numerics follow the reference's CPU torch kernels so that results agree to ~1 ulp:
//   * cumprod / cumsum accumulate float inputs in fp64 and round every prefix to fp32;
//   * position and depth arithmetic is separate mul + add (the file is built with -ffp-contract=off);
//   * searchsorted(right=True) = number of CDF entries <= u.
#include "device_common.h"
#include "host_common.h"
#include "../../include/nerf_amd.h"
#include "launchers.h"

extern __shared__ __attribute__((aligned(16))) char smem[];

namespace {

constexpr int WAVES_PER_BLOCK = 4;

DEVINL int wave_in_block() { return (int)(threadIdx.x >> 6); }

// ---------------------------------------------------------------------------------------- rows 3 and 12: the stand-alone encoders
// Both are HBM-bound by their OUTPUT (24 L bytes per sample against 12-30 read): a workgroup takes ENC_TILE samples,
//   phase 1  one thread per sample parks the encoder's per-coordinate inputs in LDS (PE: x; IPE: Gaussian mean and diagonal covariance);
//   phase 2  one thread per (sample, frequency, coordinate) PAIR evaluates sin and cos from one range reduction (and, for the IPE, one
//            exp shared by both) and stages the two values in LDS in output order;
//   phase 3  the tile's 24 L ENC_TILE bytes leave as fully coalesced 16-byte stores.
// The first version computed every output element on its own (one range reduction per element, a 64-bit division per element, 4-byte
// stores): 0.2 TB/s (PE) / 2.0 TB/s (IPE) at 640 000 x 128 samples.
constexpr int ENC_TILE = 64;                          // dynamic LDS: ENC_TILE x (6 L staged outputs + 6 moments) floats = 16.5 KiB at L = 10
static inline size_t enc_lds_bytes(int L) { return (size_t)ENC_TILE * (6 * L + 6) * 4; }
template <bool IPE, class Moments>
DEVINL void encode_tile(float (*mom)[6], float* stage, int64_t base, int64_t total, int L, float* __restrict__ feat, Moments&& moments) {
    const int width = 6 * L, pairs_per = 3 * L;
    const int nsamp = (int)(total - base < ENC_TILE ? total - base : ENC_TILE);
    if ((int)threadIdx.x < nsamp) moments((int)threadIdx.x, base + threadIdx.x);
    __syncthreads();
    const int n_pairs = nsamp * pairs_per;
    for (int p = threadIdx.x; p < n_pairs; p += blockDim.x) {
        const int sl = p / pairs_per, rem = p - sl * pairs_per;
        const int l = rem / 3, c = rem - 3 * l;
        float sn, cs;
        sincos_quadrant(mom[sl][c] * (float)(1 << l), sn, cs);                        // exact scaling (nerf_helper.py:42-44, mip_methods.py:43)
        if (IPE) {
            const float e = expf(-0.5f * (mom[sl][3 + c] * (float)(1u << (2 * l))));  // diag_P * diag (mip_methods.py:42,55)
            sn *= e; cs *= e;
        }
        stage[sl * width + 6 * l + c] = sn;
        stage[sl * width + 6 * l + 3 + c] = cs;
    }
    __syncthreads();
    const int cnt = nsamp * width;
    float* o = feat + base * width;                                                     // (base * width * 4 is a multiple of 16)
    const f32x4* s4 = reinterpret_cast<const f32x4*>(stage);
    f32x4* o4 = reinterpret_cast<f32x4*>(o);
    for (int i = threadIdx.x; i < cnt / 4; i += blockDim.x) o4[i] = s4[i];
    for (int i = (cnt & ~3) + threadIdx.x; i < cnt; i += blockDim.x) o[i] = stage[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void pe_kernel(const float* __restrict__ x, int64_t M, int L, float* __restrict__ out) {
    float* stage = reinterpret_cast<float*>(smem);
    float (*mom)[6] = reinterpret_cast<float (*)[6]>(stage + ENC_TILE * 6 * L);
    for (int64_t base = blockIdx.x * (int64_t)ENC_TILE; base < M; base += (int64_t)gridDim.x * ENC_TILE)
        encode_tile<false>(mom, stage, base, M, L, out, [&](int sl, int64_t m) {
            mom[sl][0] = x[m * 3]; mom[sl][1] = x[m * 3 + 1]; mom[sl][2] = x[m * 3 + 2];
        });
}

// Integrated positional encoding (mip_methods.py:15-58): the Gaussian moments of the frustum (cone_moments / cone_mean_cov,
// device_common.h: the reference's operation order), then
//   out[.., 6 l + 3 t + c] = (t ? cos : sin)(2^l mu_c) * exp(-0.5 * (4^l diag_c))     (multFreq :36-45, ipe_feature :51-58)
__global__ __launch_bounds__(256) void ipe_feature_kernel(const float* __restrict__ z, const float* __restrict__ rays, int64_t N, int S, int L,
                                                           float r2, const float* __restrict__ dir_norm, float* __restrict__ feat,
                                                           float* __restrict__ mu_out, float* __restrict__ mu_t_out, int contract) {
    float* stage = reinterpret_cast<float*>(smem);
    float (*mom)[6] = reinterpret_cast<float (*)[6]>(stage + ENC_TILE * 6 * L);
    const int64_t total = N * S;
    const float dn = dir_norm[0];
    for (int64_t base = blockIdx.x * (int64_t)ENC_TILE; base < total; base += (int64_t)gridDim.x * ENC_TILE)
        encode_tile<true>(mom, stage, base, total, L, feat, [&](int sl, int64_t m) {
            const int64_t n = m / S;
            const int si = (int)(m - n * S);
            const float* zz = z + n * (S + 1) + si;
            const ConeMoments c = cone_moments(zz[0], zz[1], r2);
            const float* ry = rays + n * 6;
            if (contract == NERF_AMD_CONTRACT_GAUSSIAN) {    // the whole Gaussian through the contraction: the function of the fused kernels' sample fetch
                float mu[3], var[3];
                cone_mean_cov_gaussian(c, ry, ry + 3, dn, mu, var);
#pragma unroll
                for (int k = 0; k < 3; ++k) { mom[sl][k] = mu[k]; mom[sl][3 + k] = var[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) cone_mean_cov(c, ry[k], ry[3 + k], dn, mom[sl][k], mom[sl][3 + k]);
                if (contract) {                              // Mip-NeRF 360 contraction of the frustum MEAN (the covariance stays metric): the fused
                    const float nn = norm3(mom[sl][0], mom[sl][1], mom[sl][2]);   // kernels' sample fetch does the same (mlp_kernels.hip contract_position)
                    if (nn > 1.0f) {
                        const float kk = (2.0f - 1.0f / nn) / nn;
                        mom[sl][0] *= kk; mom[sl][1] *= kk; mom[sl][2] *= kk;
                    }
                }
            }
            if (mu_out) { mu_out[m * 3] = mom[sl][0]; mu_out[m * 3 + 1] = mom[sl][1]; mu_out[m * 3 + 2] = mom[sl][2]; }
            if (mu_t_out) mu_t_out[m] = c.mu_t;
        });
}

// coneParameters alone (mip_methods.py:15-23): z (N, S+1) -> mu_t, sigma_t^2, sigma_r^2 (N, S)
__global__ void cone_parameters_kernel(const float* __restrict__ z, int64_t N, int S, float r2, float* __restrict__ mu_t, float* __restrict__ var_t,
                                       float* __restrict__ var_r) {
    const int64_t total = N * S;
    for (int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; m < total; m += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = m / S;
        const float* zz = z + n * (S + 1) + (m - n * S);
        const ConeMoments c = cone_moments(zz[0], zz[1], r2);
        mu_t[m] = c.mu_t; var_t[m] = c.var_t; var_r[m] = c.var_r;
    }
}

// norm of the whole direction tensor (mip_methods.py:31 `cam_rays[:, 3:].norm()`): one workgroup, fp64 partial sums, fixed order
__global__ __launch_bounds__(1024) void dirs_norm_kernel(const float* __restrict__ rays, int64_t N, float* __restrict__ out) {
    __shared__ double part[1024];
    double acc = 0.0;
    for (int64_t n = threadIdx.x; n < N; n += 1024) {
        const float* d = rays + n * 6 + 3;
        acc += (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sqrt(part[0]);
}

// the same over the whole chip when the caller has scratch for the workgroup partials (the render path: 0.36 ms -> a few microseconds per
// 640 000 rays): fp64 partial sums per workgroup, then one workgroup adds the partials in a fixed order
constexpr int DN_BLOCKS = 256;
__global__ __launch_bounds__(256) void dirs_norm_partial_kernel(const float* __restrict__ rays, int64_t N, double* __restrict__ partials) {
    __shared__ double part[256];
    double acc = 0.0;
    for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)DN_BLOCKS * 256) {
        const float* d = rays + n * 6 + 3;
        acc += (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = part[0];
}
__global__ __launch_bounds__(256) void dirs_norm_final_kernel(const double* __restrict__ partials, float* __restrict__ out) {
    __shared__ double part[256];
    part[threadIdx.x] = partials[threadIdx.x];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sqrt(part[0]);
}

// ---------------------------------------------------------------------------------------- row 1
struct Cam { int H, W; float fx, fy; float pose[12]; };

// The ray (o, d) through camera-plane coordinates (cx, cy) of a (3,4) pose, and the point o + z d on a ray: the one definition of each for
// every kernel of this file that forms them (same expression grouping, so the kernels agree bit for bit where they overlap).
DEVINL void camera_ray(const float* pose, float cx, float cy, float* r) {
    r[0] = pose[3]; r[1] = pose[7]; r[2] = pose[11];
    r[3] = (cx * pose[0] + cy * pose[1]) + (-1.0f) * pose[2];
    r[4] = (cx * pose[4] + cy * pose[5]) + (-1.0f) * pose[6];
    r[5] = (cx * pose[8] + cy * pose[9]) + (-1.0f) * pose[10];
}
DEVINL void point_on_ray(const float* r, float z, float* p) {
    p[0] = r[0] + r[3] * z; p[1] = r[1] + r[4] * z; p[2] = r[2] + r[5] * z;
}

__global__ void raygen_kernel(Cam cam, int64_t first, int64_t count, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = first + i;
        float* rays = out - first * 6;
        const int row = (int)(n / cam.W), col = (int)(n - (int64_t)row * cam.W);
        const float cx = (((float)col - (float)cam.W * 0.5f) + 0.5f) / cam.fx;
        const float cy = (((float)cam.H * 0.5f - (float)row) + 0.5f) / cam.fy;
        camera_ray(cam.pose, cx, cy, rays + n * 6);
    }
}

// training twin of row 1 (utils.py:78-85): integer (col - W//2, H//2 - row) coords -> rays
__global__ void pixel_rays_kernel(Cam cam, const int64_t* __restrict__ coords, int64_t N, float* __restrict__ rays) {
    for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const float cx = ((float)coords[n * 2] + 0.5f) / cam.fx;
        const float cy = ((float)coords[n * 2 + 1] + 0.5f) / cam.fy;
        camera_ray(cam.pose, cx, cy, rays + n * 6);
    }
}

// ---------------------------------------------------------------------------------------- camera model (include/nerf_amd.h)
// A camera row of NERF_AMD_CAMERA_ROW floats: fx fy cx cy k1 k2 k3 p1 p2 (+ reserved zeros).  The one definition of pixel -> ray for every
// kernel that takes a camera row: the distorted image-plane point of the pixel centre, COLMAP's convention, then the OpenCV model
//   xd = x rad + 2 p1 x y + p2 (r2 + 2 x^2),  yd = y rad + 2 p2 x y + p1 (r2 + 2 y^2),  rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
// solved for (x, y) by NERF_AMD_CAMERA_NEWTON_STEPS Newton steps from (xd, yd) with the analytic Jacobian (a step whose |det| is below
// NERF_AMD_CAMERA_DET_EPS is skipped); all five coefficients zero: no step, (x, y) = (xd, yd) exactly.  Plain mul / add / div in the
// order written (the build contracts nothing): tests/camera_ref.py restates it operation by operation.
struct CameraRow { float v[NERF_AMD_CAMERA_ROW]; };
DEVINL void pixel_camera_ray(int col, int row, const float* cam, const float* pose, float* r) {
    const float fx = cam[0], fy = cam[1], k1 = cam[4], k2 = cam[5], k3 = cam[6], p1 = cam[7], p2 = cam[8];
    const float xd = (((float)col + 0.5f) - cam[2]) / fx;
    const float yd = (((float)row + 0.5f) - cam[3]) / fy;
    float x = xd, y = yd;
    if (k1 != 0.0f || k2 != 0.0f || k3 != 0.0f || p1 != 0.0f || p2 != 0.0f) {
#pragma unroll 1
        for (int it = 0; it < NERF_AMD_CAMERA_NEWTON_STEPS; ++it) {
            const float xx = x * x, yy = y * y, xy = x * y;
            const float r2 = xx + yy;
            const float rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
            const float drad = k1 + r2 * (2.0f * k2 + r2 * (3.0f * k3));                 // d rad / d r2
            const float ex = ((x * rad + (2.0f * p1) * xy) + p2 * (r2 + 2.0f * xx)) - xd;
            const float ey = ((y * rad + (2.0f * p2) * xy) + p1 * (r2 + 2.0f * yy)) - yd;
            const float jxx = ((rad + (2.0f * xx) * drad) + (2.0f * p1) * y) + (6.0f * p2) * x;
            const float jyy = ((rad + (2.0f * yy) * drad) + (2.0f * p2) * x) + (6.0f * p1) * y;
            const float jxy = ((2.0f * xy) * drad + (2.0f * p1) * x) + (2.0f * p2) * y;   // = d ex / d y = d ey / d x
            const float det = jxx * jyy - jxy * jxy;
            if (!(fabsf(det) >= NERF_AMD_CAMERA_DET_EPS)) continue;
            x = x - (jyy * ex - jxy * ey) / det;
            y = y - (jxx * ey - jxy * ex) / det;
        }
    }
    camera_ray(pose, x, -y, r);
}

// row 1 for one camera row: raygen_kernel's indexing (rays n = row W + col of [first, first + count)); the camera travels in the launch
// arguments, so its reads are wave-uniform
__global__ __launch_bounds__(256) void raygen_camera_kernel(CameraRow cam, Cam pose, int64_t first, int64_t count, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = first + i;
        const int row = (int)(n / pose.W), col = (int)(n - (int64_t)row * pose.W);
        float r[6];
        pixel_camera_ray(col, row, cam.v, pose.pose, r);
#pragma unroll
        for (int k = 0; k < 6; ++k) out[i * 6 + k] = r[k];
    }
}

// row 2 (utils.py:87-90 / procedures.py:65-66): z = z_base + u*jitter ; pts = o + d*z
__global__ void stratified_points_kernel(const float* __restrict__ rays, const float* __restrict__ z_base,
                                         const float* __restrict__ u, float jitter, int64_t N, int S,
                                         float* __restrict__ z_out, float* __restrict__ pts) {
    const int64_t total = N * S;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / S;
        const int s = (int)(i - n * S);
        const float zv = z_base[s] + u[i] * jitter;
        z_out[i] = zv;
        if (pts) point_on_ray(rays + n * 6, zv, pts + i * 3);
    }
}

// ---------------------------------------------------------------------------------------- training sampler
// validSampler (utils.py:72-94) in ONE launch with every random number drawn in the kernel: pixel index of ray n = floor(P * u) from
// Philox stream 'IX', ground-truth colour gather, ray through the pixel (utils.py:78-85), stratified depths z = base_s + u * res from
// stream 'TS' (utils.py:87-89) and the sample positions o + d z (utils.py:90).  The reference draws both on the CPU generator and
// copies them to the device every iteration (train.py:153-157).  One workgroup = 4 rays x C samples.
constexpr uint32_t PHILOX_STREAM_INDEX = 0x4958u, PHILOX_STREAM_TRAIN = 0x5453u;
// The per-ray and per-sample bodies, shared by train_sampler_kernel and scene_sampler_kernel (same words, same expression grouping: the
// two kernels agree bit for bit where they overlap).
// 64-bit word of counter (n, 0, 'IX'): floor(P * x / 2^64) is ray n's uniform draw in [0, P)
DEVINL uint64_t sampler_index_word(int64_t n, uint64_t seed) {
    const Philox4 r = philox4x32_10((uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0u, PHILOX_STREAM_INDEX, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ((uint64_t)r.w[0] << 32) | r.w[1];
}
// ray through the pixel with integer coordinates (ix, iy) = (col - W//2, H//2 - row) (utils.py:78-85) -> q[6] (LDS) and rays[n]
DEVINL void sampler_ray(const float* pose, float fx, float fy, float ix, float iy, float* q, float* __restrict__ ray_out) {
    const float cx = (ix + 0.5f) / fx;                                                   // utils.py:78-81
    const float cy = (iy + 0.5f) / fy;
    camera_ray(pose, cx, cy, q);
#pragma unroll
    for (int k = 0; k < 6; ++k) ray_out[k] = q[k];
}
// the stratified depths and positions of the (up to) 4 rays n0 .. n0+3 of a workgroup, 256 threads over 4 x C samples
DEVINL void sampler_samples(int64_t n0, int64_t N, int C, uint64_t seed, float near, float res, const float (*ray_s)[6], float* __restrict__ lengths,
                            float* __restrict__ pts) {
    const int64_t cnt = ((N - n0 < 4) ? N - n0 : 4) * C;
    for (int64_t i = threadIdx.x; i < cnt; i += 256) {
        const int rl = (int)(i / C), sidx = (int)(i - (int64_t)rl * C);
        const int64_t n = n0 + rl;
        const Philox4 r = philox4x32_10((uint32_t)n, (uint32_t)((uint64_t)n >> 32), (uint32_t)(sidx >> 2), PHILOX_STREAM_TRAIN, (uint32_t)seed,
                                        (uint32_t)(seed >> 32));
        const int w = sidx & 3;
        const float u = u01_from_bits(w == 0 ? r.w[0] : (w == 1 ? r.w[1] : (w == 2 ? r.w[2] : r.w[3])));
        const float z = (near + (float)sidx * res) + u * res;                        // linspace(near, far - res, C)[s] + u res
        lengths[n * C + sidx] = z;
        point_on_ray(ray_s[rl], z, pts + (n * C + sidx) * 3);
    }
}
// `pose_dev` / `seed_dev` (both optional): the camera pose and the seed read from DEVICE memory instead of the launch arguments, so that
// a captured hipGraph of the training step sees a new image pose and fresh random numbers on every replay.
__global__ __launch_bounds__(256) void train_sampler_kernel(const float* __restrict__ rgbs, const int64_t* __restrict__ coords, int64_t P, Cam cam,
                                                            float near, float res, int64_t N, int C, uint64_t seed, float* __restrict__ pts,
                                                            float* __restrict__ lengths, float* __restrict__ rgb, float* __restrict__ rays,
                                                            const float* __restrict__ pose_dev, const uint64_t* __restrict__ seed_dev) {
    __shared__ float ray_s[4][6];
    if (pose_dev != nullptr) {
#pragma unroll
        for (int i = 0; i < 12; ++i) cam.pose[i] = pose_dev[i];
    }
    if (seed_dev != nullptr) seed = seed_dev[0];
    for (int64_t n0 = blockIdx.x * (int64_t)4; n0 < N; n0 += (int64_t)gridDim.x * 4) {
        __syncthreads();
        if (threadIdx.x < 4 && n0 + threadIdx.x < N) {
            const int64_t n = n0 + threadIdx.x;
            const int64_t idx = (int64_t)__umul64hi(sampler_index_word(n, seed), (uint64_t)P);     // uniform in [0, P)
            sampler_ray(cam.pose, cam.fx, cam.fy, (float)coords[idx * 2], (float)coords[idx * 2 + 1], ray_s[threadIdx.x], rays + n * 6);
#pragma unroll
            for (int k = 0; k < 3; ++k) rgb[n * 3 + k] = rgbs[idx * 3 + k];
        }
        __syncthreads();
        if (lengths == nullptr) continue;
        sampler_samples(n0, N, C, seed, near, res, ray_s, lengths, pts);
    }
}

// The scene twin: the batch drawn uniformly over the window of K views of a planar image stack images (V,3,H,W), read in place -- no
// (H W, 3) pixel table, no coordinate table -- with each ray's pose fetched from poses (V,3,4).  cell = floor(K wp * x / 2^64) with x the
// word train_sampler_kernel draws; view slot k = cell / wp, and the remainder enumerates the window row-major like randomFromOneImage's
// table, so K = 1 reproduces train_sampler_kernel on that table bit for bit.  Every index here is 64-bit by construction: K wp and
// V H W are never assumed to fit 32 bits (a stack of that size cannot be allocated for a test).  A view id outside [0, V) (a device
// tensor the host never saw) reads nothing: that ray is NaN with index -1.
__global__ __launch_bounds__(256) void scene_sampler_kernel(const float* __restrict__ images, const float* __restrict__ poses, int64_t V, int H, int W,
                                                            const int64_t* __restrict__ view_ids, int64_t K, int x0, int ww, int y0, int64_t wp,
                                                            float fx, float fy, float near, float res, int64_t N, int C, uint64_t seed,
                                                            const uint64_t* __restrict__ seed_dev, float* __restrict__ pts, float* __restrict__ lengths,
                                                            float* __restrict__ rgb, float* __restrict__ rays, int64_t* __restrict__ index) {
    __shared__ float ray_s[4][6];
    if (seed_dev != nullptr) seed = seed_dev[0];
    const uint64_t P = (uint64_t)K * (uint64_t)wp;
    for (int64_t n0 = blockIdx.x * (int64_t)4; n0 < N; n0 += (int64_t)gridDim.x * 4) {
        __syncthreads();
        if (threadIdx.x < 4 && n0 + threadIdx.x < N) {
            const int64_t n = n0 + threadIdx.x;
            const int64_t cell = (int64_t)__umul64hi(sampler_index_word(n, seed), P);               // uniform in [0, K wp)
            const int64_t k = cell / wp, r = cell - k * wp;
            const int64_t wr = r / ww;
            const int64_t row = y0 + wr, col = x0 + (r - wr * ww);
            const int64_t v = view_ids != nullptr ? view_ids[k] : k;
            float* q = ray_s[threadIdx.x];
            if (v >= 0 && v < V) {
                sampler_ray(poses + v * 12, fx, fy, (float)(col - W / 2), (float)(H / 2 - row), q, rays + n * 6);
                const float* px = images + ((v * 3) * (int64_t)H + row) * W + col;
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[n * 3 + c] = px[(int64_t)c * H * W];
                if (index != nullptr) index[n] = (v * H + row) * W + col;
            } else {
                const float nan = __builtin_nanf("");
#pragma unroll
                for (int c = 0; c < 6; ++c) { q[c] = nan; rays[n * 6 + c] = nan; }
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[n * 3 + c] = nan;
                if (index != nullptr) index[n] = -1;
            }
        }
        __syncthreads();
        if (lengths == nullptr) continue;
        sampler_samples(n0, N, C, seed, near, res, ray_s, lengths, pts);
    }
}

// The camera twin of scene_sampler_kernel: view v's ray goes through pixel_camera_ray with row v of `cameras` (V, NERF_AMD_CAMERA_ROW), a
// DEVICE table read when the kernel runs (a captured step replays with it).  Everything else is scene_sampler_kernel's: the same Philox
// words, cell -> (view, row, col) decode, window, view_ids, NaN / -1 for a view id outside [0, V), index and stratified depths.
__global__ __launch_bounds__(256) void scene_sampler_camera_kernel(const float* __restrict__ images, const float* __restrict__ poses,
                                                                   const float* __restrict__ cameras, int64_t V, int H, int W,
                                                                   const int64_t* __restrict__ view_ids, int64_t K, int x0, int ww, int y0, int64_t wp,
                                                                   float near, float res, int64_t N, int C, uint64_t seed,
                                                                   const uint64_t* __restrict__ seed_dev, float* __restrict__ pts, float* __restrict__ lengths,
                                                                   float* __restrict__ rgb, float* __restrict__ rays, int64_t* __restrict__ index) {
    __shared__ float ray_s[4][6];
    if (seed_dev != nullptr) seed = seed_dev[0];
    // the key lives in vector registers: as a wave-uniform value Philox's whole key schedule (two words for each of ten rounds) is hoisted
    // into scalar registers, which with this argument list spills some of them (the same words come out either way)
    asm volatile("" : "+v"(seed));
    const uint64_t P = (uint64_t)K * (uint64_t)wp;
    for (int64_t n0 = blockIdx.x * (int64_t)4; n0 < N; n0 += (int64_t)gridDim.x * 4) {
        __syncthreads();
        if (threadIdx.x < 4 && n0 + threadIdx.x < N) {
            const int64_t n = n0 + threadIdx.x;
            const int64_t cell = (int64_t)__umul64hi(sampler_index_word(n, seed), P);               // uniform in [0, K wp)
            const int64_t k = cell / wp, r = cell - k * wp;
            const int64_t wr = r / ww;
            const int64_t row = y0 + wr, col = x0 + (r - wr * ww);
            const int64_t v = view_ids != nullptr ? view_ids[k] : k;
            float* q = ray_s[threadIdx.x];
            if (v >= 0 && v < V) {
                pixel_camera_ray((int)col, (int)row, cameras + v * NERF_AMD_CAMERA_ROW, poses + v * 12, q);
                const float* px = images + ((v * 3) * (int64_t)H + row) * W + col;
#pragma unroll
                for (int c = 0; c < 6; ++c) rays[n * 6 + c] = q[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[n * 3 + c] = px[(int64_t)c * H * W];
                if (index != nullptr) index[n] = (v * H + row) * W + col;
            } else {
                const float nan = __builtin_nanf("");
#pragma unroll
                for (int c = 0; c < 6; ++c) { q[c] = nan; rays[n * 6 + c] = nan; }
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[n * 3 + c] = nan;
                if (index != nullptr) index[n] = -1;
            }
        }
        __syncthreads();
        if (lengths == nullptr) continue;
        sampler_samples(n0, N, C, seed, near, res, ray_s, lengths, pts);
    }
}

// ---------------------------------------------------------------------------------------- row 8
__global__ void length2pts_kernel(const float* __restrict__ rays, const float* __restrict__ z, int64_t N, int S,
                                  float* __restrict__ out) {
    const int64_t total = N * S * 6;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ns = i / 6;
        const int k = (int)(i - ns * 6);
        const int64_t n = ns / S;
        const float* r = rays + n * 6;
        out[i] = (k < 3) ? (r[k] + r[3 + k] * z[ns]) : r[k];
    }
}

__global__ __launch_bounds__(256) void sigma_to_weights_kernel(const float* __restrict__ sigma, const float* __restrict__ z,
                                                              const float* __restrict__ dirs, int64_t N, int S, int act,
                                                              float* __restrict__ w) {
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        float nrm = 1.0f;
        const bool scale = dirs != nullptr;
        if (scale) nrm = norm3(dirs[n * 3], dirs[n * 3 + 1], dirs[n * 3 + 2]);
        const float* sg = sigma + n * S;
        const float* zz = z + n * S;
        float* wo = w + n * S;
        wave_sigma_to_weights(S, act, [&](int s) { return sg[s]; },
                              [&](int s) { return scale ? zz[s] * nrm : zz[s]; },
                              [&](int s, float wv, float) { wo[s] = wv; });
    }
}

// ---------------------------------------------------------------------------------------- row 6
// element s of maxBlurFilter (mip_methods.py:61-66) over the row w[0 .. S-1]; the row's ends see themselves
DEVINL float max_blur_at(const float* w, int s, int S, float alpha) {
    const float c = w[s];
    const float front = (s == 0) ? c : fmaxf(w[s - 1], c);
    const float rear = (s == S - 1) ? c : fmaxf(c, w[s + 1]);
    return 0.5f * (front + rear) + alpha;
}
__global__ void max_blur_kernel(const float* __restrict__ w, int64_t N, int S, float alpha, float* __restrict__ out) {
    const int64_t total = N * S;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(i % S);
        out[i] = max_blur_at(w + (i - s), s, S, alpha);
    }
}

// ------------------------------------------------------------------------------------------------
// Inverse-transform sampling for one ray by one wavefront (row 7, utils.py:108-133).
//   pw[nw]   raw pdf weights (1e-5 is added here), bins[nw+1] bin edges -- both in LDS, visible to the wave
//   cdf[nw+1], samp[K], bel[K]: LDS scratch
// ------------------------------------------------------------------------------------------------
DEVINL void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#ifndef SORT_NB_DEF
#define SORT_NB_DEF 256
#define SORT_CAP_DEF 6
#endif
constexpr int SORT_NB = SORT_NB_DEF, SORT_CAP = SORT_CAP_DEF, SORT_PER_LANE = SORT_NB / 64;
constexpr int SORT_LDS_FLOATS = 2 * SORT_NB + SORT_NB * SORT_CAP / 2;      // cnt, pre (int) + members (uint16)

// uf(i, k) = the uniform of sample k = lane + 64 i (a global pointer, or registers loaded one ray ahead)
template <class UF>
DEVINL void wave_inverse_sample(const float* pw, const float* bins, int nw, float* cdf, float* samp, int* bel, int* sortbuf,
                                UF&& uf, int K, int sort, float* __restrict__ z_out,
                                int64_t* __restrict__ below_out, int64_t* __restrict__ above_out) {
    const int lane = lane_id();
    const int nb = nw + 1;           // bins == cdf entries incl. the leading 0
    // pdf normaliser torch.sum(weights + 1e-5, -1) (utils.py:110-111) in the summation ORDER of torch's CPU kernel, so that the CDF --
    // and with it every searchsorted decision -- is bit-identical to the reference's.  ATen's cascade_sum over a contiguous row
    // (SumKernel.cpp vectorized_inner_sum; verified against torch 2.10 for row lengths 14..255, tests/test_oracle_golden.py): the row is
    // read as 8-float vectors, vector v goes to accumulator v % 4 while whole groups of four remain and to accumulator 0 afterwards,
    // accumulators 1..3 are added to 0 in order; the scalar result is 0 + the < 8 tail elements in order + the 8 vector slots in order.
    // (Rows of >= 512 elements add cascade levels; nw < 256 here.)
    float* part8 = reinterpret_cast<float*>(sortbuf);             // the sort scratch is free until the sort
    const int nv = nw >> 3;
    if (lane < 8) {
        const int n4 = nv >> 2;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int i = 0; i < n4; ++i) {
            a0 += pw[32 * i + lane] + 1e-5f;
            a1 += pw[32 * i + 8 + lane] + 1e-5f;
            a2 += pw[32 * i + 16 + lane] + 1e-5f;
            a3 += pw[32 * i + 24 + lane] + 1e-5f;
        }
        for (int v = 4 * n4; v < nv; ++v) a0 += pw[8 * v + lane] + 1e-5f;
        a0 += a1; a0 += a2; a0 += a3;
        part8[lane] = a0;
    }
    lds_wave_sync();
    float total = 0.0f;              // every lane forms the same scalar (LDS broadcast reads)
    if (nv > 0) {
        for (int j = 8 * nv; j < nw; ++j) total += pw[j] + 1e-5f;
#pragma unroll
        for (int c = 0; c < 8; ++c) total += part8[c];
    } else {                         // rows shorter than one vector: the scalar form (4 accumulators over single elements)
        float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        if (nw >= 4) { total += pw[0] + 1e-5f; a1 += pw[1] + 1e-5f; a2 += pw[2] + 1e-5f; a3 += pw[3] + 1e-5f; }
        for (int j = nw & ~3; j < nw; ++j) total += pw[j] + 1e-5f;
        total += a1; total += a2; total += a3;
    }
    // cdf: fp64 running sum of fp32 pdf values, rounded per element (torch CPU cumsum)
    double carry = 0.0;
    if (lane == 0) cdf[0] = 0.0f;
    for (int base = 0; base < nw; base += 64) {
        const int j = base + lane;
        double p = 0.0;
        if (j < nw) p = (double)((pw[j] + 1e-5f) / total);
        const double incl = wave_incl_scan_add(p);
        if (j < nw) cdf[1 + j] = (float)(carry + incl);
        carry += wave_last(incl);
    }
    lds_wave_sync();
    // searchsorted(right=True): count of cdf entries <= u.  Three samples per lane (K <= 192: all of the ray's) are searched in
    // lock step with a fixed trip count, so that their dependent LDS reads overlap instead of running back to back.
    const int halvings = 32 - __builtin_clz((unsigned)nb);       // an interval of nb + 1 candidates is empty after that many steps
    for (int k0 = 0, i0 = 0; k0 < K; k0 += 192, i0 += 3) {
        float uu[3]; int lo[3], hi[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = k0 + 64 * q + lane;
            uu[q] = (k < K) ? uf(i0 + q, k) : 0.0f;
            lo[q] = 0; hi[q] = (k < K) ? nb : 0;
        }
        for (int it = 0; it < halvings; ++it) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int mid = (lo[q] + hi[q]) >> 1;
                const bool open_ = lo[q] < hi[q];
                const float c = cdf[open_ ? mid : 0];
                if (open_) { if (c <= uu[q]) lo[q] = mid + 1; else hi[q] = mid; }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = k0 + 64 * q + lane;
            if (k >= K) continue;
            const int below = lo[q] - 1 > 0 ? lo[q] - 1 : 0;
            const int above = lo[q] < nb - 1 ? lo[q] : nb - 1;
            const float c0 = cdf[below], c1 = cdf[above];
            float denom = c1 - c0;
            if (denom < 1e-5f) denom = 1.0f;
            const float t = (uu[q] - c0) / denom;
            const float b0 = bins[below], b1 = bins[above];
            const float v = b0 + t * (b1 - b0);
            if (sort) { samp[k] = v; bel[k] = below; }
            else {
                z_out[k] = v;
                if (below_out) below_out[k] = below;
                if (above_out) above_out[k] = above;
            }
        }
    }
    if (!sort) return;
    lds_wave_sync();
    // Sort BY VALUE, like torch.sort.  Inside one bin every fp32 operation of the interpolation is monotone in u and a bin's samples
    // start at its lower edge b0, so over ascending bin edges the order of the samples is the order of their uniforms AS LONG AS no
    // sample exceeds its own upper edge b1.  In fp32 one can: for u one ulp below cdf[above], t rounds to 1 and b0 + fl(b1 - b0)
    // exceeds b1 by an ulp when the width b1 - b0 is not exact, while the next uniform, on the edge, gives b1 itself -- a descent, and
    // across a bucket boundary one that the bucket sort would keep.  Where the width IS exact (0 <= b0 <= b1 <= 2 b0, or the mirror
    // image below zero: Sterbenz) t <= 1 gives fl(t w) <= w and b0 + fl(t w) <= b1.  So: a ray none of whose bins is `risky` is sorted
    // by its uniforms -- bucket the elements by floor(u * 256) (LDS atomics hand out the slot inside a bucket), prefix-sum the bucket
    // counts, and rank every element against the <= SORT_CAP members of its own bucket only -- and a ray with risky bins first looks
    // for a sample above its upper edge among the samples of those bins.  Such a ray, and a ray with more than SORT_CAP elements in
    // one bucket, takes the O(K^2) stable rank sort; both sorts give the same sorted values.
    int* cnt = sortbuf;
    int* pre = sortbuf + SORT_NB;
    unsigned short* mem = reinterpret_cast<unsigned short*>(sortbuf + 2 * SORT_NB);
    for (int b = lane; b < SORT_NB; b += 64) cnt[b] = 0;
    lds_wave_sync();
    // (the order-of-uniforms argument needs ascending bin edges; a ray whose edges are not -- unsorted depths passed to inverseSample,
    // or stratified depths whose jitter exceeds the bin spacing -- takes the rank sort below, which sorts the VALUES like torch.sort)
    int overflow = 0, risky = -1;                 // risky: this lane's last bin whose width is not exact in fp32
    for (int j = lane; j + 1 < nb; j += 64) {
        const float b0 = bins[j], b1 = bins[j + 1];
        overflow |= (b1 < b0) ? 1 : 0;
        const bool exact = b0 >= 0.0f ? (b1 <= 2.0f * b0 || b0 == 0.0f) : (b1 <= 0.0f && b0 >= 2.0f * b1);
        if (!exact) risky = j;
    }
    if (__any(risky >= 0)) {                      // (never on metric depths a factor of two apart at most; bin 0 under disparity spacing)
        risky = wave_max_i(risky);
        for (int k = lane; k < K; k += 64) {
            const int bl = bel[k];                // bl <= risky < nb - 1: the upper edge is bins[bl + 1]
            if (bl <= risky) overflow |= (samp[k] > bins[bl + 1]) ? 1 : 0;
        }
    }
    for (int k = lane, i = 0; k < K; k += 64, ++i) {
        int b = (int)(uf(i, k) * (float)SORT_NB);
        b = b < 0 ? 0 : (b > SORT_NB - 1 ? SORT_NB - 1 : b);
        const int pos = atomicAdd(&cnt[b], 1);
        if (pos < SORT_CAP) mem[b * SORT_CAP + pos] = (unsigned short)k; else overflow = 1;
    }
    lds_wave_sync();
    if (__any(overflow)) {
        for (int k = lane; k < K; k += 64) {          // stable rank sort (LDS broadcast reads)
            const float v = samp[k];
            int rank = 0;
            for (int j = 0; j < K; ++j) {
                const float o = samp[j];
                rank += (o < v || (o == v && j < k)) ? 1 : 0;
            }
            z_out[rank] = v;
            if (below_out) below_out[rank] = bel[k];
        }
        return;
    }
    {   // exclusive prefix sum of the SORT_NB bucket counts: SORT_NB / 64 per lane (128 x 8, 128 x 6 and 64 x 12 layouts measured slower: more rank work per bucket than the extra occupancy pays)
        int c[SORT_PER_LANE], tot = 0;
#pragma unroll
        for (int i = 0; i < SORT_PER_LANE; ++i) { c[i] = cnt[lane * SORT_PER_LANE + i]; tot += c[i]; }
        int run = wave_incl_scan_add(tot) - tot;
#pragma unroll
        for (int i = 0; i < SORT_PER_LANE; ++i) { pre[lane * SORT_PER_LANE + i] = run; run += c[i]; }
    }
    lds_wave_sync();
    for (int k0 = 0, i0 = 0; k0 < K; k0 += 192, i0 += 3) {          // three elements per lane in lock step (dependent LDS reads overlap)
        float v[3]; int rank[3], cntb[3], bb[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = k0 + 64 * q + lane;
            const bool ok = k < K;
            int b = ok ? (int)(uf(i0 + q, k) * (float)SORT_NB) : 0;
            b = b < 0 ? 0 : (b > SORT_NB - 1 ? SORT_NB - 1 : b);
            bb[q] = b;
            v[q] = samp[ok ? k : 0];
            rank[q] = pre[b];
            cntb[q] = ok ? cnt[b] : 0;
        }
        int most = cntb[0] > cntb[1] ? cntb[0] : cntb[1];
        most = most > cntb[2] ? most : cntb[2];
        const int trips = wave_max_i(most);                       // wave-uniform: the fullest bucket any lane looks at (typically 3..4 of SORT_CAP)
        for (int p = 0; p < trips; ++p) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int k = k0 + 64 * q + lane;
                const bool live = p < cntb[q];
                const int jx = mem[bb[q] * SORT_CAP + p];
                const float o = samp[live ? jx : 0];
                rank[q] += (live && (o < v[q] || (o == v[q] && jx < k))) ? 1 : 0;
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int k = k0 + 64 * q + lane;
            if (k >= K) continue;
            z_out[rank[q]] = v[q];
            if (below_out) below_out[rank[q]] = bel[k];
        }
    }
}

// The per-wave LDS rows of the five inverse-sampling kernels, described ONCE (all rows are 4-byte words; bel and sortbuf hold ints):
//   pw[C] bins[C] cdf[C] samp[K] bel[K] sortbuf[SORT_LDS_FLOATS] | zl[C] wraw[C] | tail
// inverse_sample_kernel ends at zl; the fused kernels add zl (metric depths) and wraw (unblurred weights) and put their own rows at `tail`.
// P = float*: the kernels' pointers from a wave's base; P = size_t: the same walk from 0 counts the floats, so the launch sizes
// (nk::sk_*_lds_bytes) cannot disagree with the carve.
template <class P> struct ResampleRowsAt { P pw, bins, cdf, samp, bel, sortbuf, zl, wraw, tail; };
typedef ResampleRowsAt<float*> ResampleRows;
template <class P> static inline __host__ __device__ ResampleRowsAt<P> resample_rows(P base, int C, int K) {
    ResampleRowsAt<P> r;
    r.pw = base; r.bins = r.pw + C; r.cdf = r.bins + C; r.samp = r.cdf + C; r.bel = r.samp + K; r.sortbuf = r.bel + K;
    r.zl = r.sortbuf + SORT_LDS_FLOATS; r.wraw = r.zl + C; r.tail = r.wraw + C;
    return r;
}
static inline __host__ __device__ size_t inv_lds_floats(int C, int K) { return resample_rows<size_t>(0, C, K).zl; }
static inline __host__ __device__ size_t rs_lds_floats(int C, int K) { return resample_rows<size_t>(0, C, K).tail; }
// tails: warped_resample_kernel sf[K] uu[K]; resample_window_kernel uu[K] | sf[K] (WARPED)
static inline __host__ __device__ size_t warped_lds_floats(int C, int K) { return rs_lds_floats(C, K) + (size_t)2 * K; }
static inline __host__ __device__ size_t rsw_lds_floats(int C, int K, bool warped) { return rs_lds_floats(C, K) + (size_t)(warped ? 2 : 1) * K; }
// the rows of this wave in a workgroup whose waves hold `wave_floats` each
DEVINL ResampleRows wave_resample_rows(size_t wave_floats, int C, int K) {
    return resample_rows(reinterpret_cast<float*>(smem) + wave_in_block() * wave_floats, C, K);
}
template <class UF>
DEVINL void wave_inverse_sample(const ResampleRows& r, int nw, UF&& uf, int K, int sort, float* __restrict__ z_out, int64_t* __restrict__ below_out,
                                int64_t* __restrict__ above_out) {
    wave_inverse_sample(r.pw, r.bins, nw, r.cdf, r.samp, reinterpret_cast<int*>(r.bel), reinterpret_cast<int*>(r.sortbuf), uf, K, sort, z_out, below_out,
                        above_out);
}

// The stages the fused resampling kernels share (one wavefront, rows in LDS; the callers put lds_wave_sync around them).
// max-blur of the raw weights (max_blur_kernel's element) -> w_prop (optional, global) and its slice [1, C-2] = the pdf row pw
DEVINL void wave_blur_pdf(const float* wraw, int C, float alpha, float* pw, float* w_prop) {
    for (int j = lane_id(); j < C; j += 64) {
        const float wb = max_blur_at(wraw, j, C, alpha);
        if (j >= 1 && j <= C - 2) pw[j - 1] = wb;                              // pdf over weights[1:-1]
        if (w_prop) w_prop[j] = wb;
    }
}
// bins[j] = the mid-point of x[j] and x[j + 1], j < C - 1
DEVINL void wave_midpoints(const float* x, int C, float* bins) {
    for (int j = lane_id(); j < C - 1; j += 64) bins[j] = 0.5f * (x[j + 1] + x[j]);
}

// mode 0: inverseSample(weights (N,C), depths (N,C)) -> bins = mid-points, pdf = weights[1:-1]   (utils.py:34-44)
// mode 1: sample_pdf(bins (N,C), weights (N,C-1))                                               (utils.py:108-133)
__global__ __launch_bounds__(256) void inverse_sample_kernel(const float* __restrict__ w, const float* __restrict__ z,
                                                            const float* __restrict__ u, int64_t N, int C, int K, int sort,
                                                            int mode, float* __restrict__ z_out, int64_t* __restrict__ below,
                                                            int64_t* __restrict__ above) {
    const ResampleRows r = wave_resample_rows(inv_lds_floats(C, K), C, K);
    float* const pw = r.pw; float* const bins = r.bins;
    const int lane = lane_id();
    const int nw = mode == 0 ? C - 2 : C - 1;
    const int wstride = mode == 0 ? C : C - 1;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        if (mode == 0) {
            for (int j = lane; j < nw; j += 64) pw[j] = w[n * wstride + 1 + j];
            wave_midpoints(z + n * C, C, bins);
        } else {
            for (int j = lane; j < nw; j += 64) pw[j] = w[n * wstride + j];
            for (int j = lane; j < nw + 1; j += 64) bins[j] = z[n * C + j];
        }
        lds_wave_sync();
        const float* un = u + n * K;
        wave_inverse_sample(r, nw, [&](int, int k) { return un[k]; }, K, sort, z_out + n * K, below ? below + n * K : nullptr,
                            above ? above + n * K : nullptr);
    }
}

// ------------------------------------------------------------------------------------------------
// Fused proposal resampling: density -> weights -> max-blur -> inverse sampling (procedures.py:68-70), i.e. wave_sigma_to_weights,
// wave_blur_pdf, wave_midpoints, wave_inverse_sample on the rows of resample_rows -- the stage functions of all four fused kernels
// (this one, warped_resample_kernel, resample_window_kernel<false / true>), which differ in where a ray's inputs and uniforms come from.
// ------------------------------------------------------------------------------------------------
struct ResampleArgs {
    const float* density; const float* z; const float* z_base; const float* u_strat; float z_jitter;
    const float* dirs; int dirs_stride; const float* u_inv; int64_t N; int C; int K; int softplus; float alpha;
    float* z_fine; int64_t* below; float* w_prop; float* z_coarse;
    uint64_t rng_seed; int64_t rng_ray_offset;      // Philox source of u_strat / u_inv when the pointers are NULL (device_common.h)
};

#ifndef RS_BLOCKS_PER_CU
#define RS_BLOCKS_PER_CU 5      /* measured: 3 -> 1.54 ms, 4 -> 1.29 ms, 5 -> 1.20 ms per 640 000 rays (96 VGPRs, 13 spilled; LDS fits 5 at the render shapes) */
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RS_BLOCKS_PER_CU, RS_BLOCKS_PER_CU))) void resample_kernel(ResampleArgs a) {
    const int C = a.C, K = a.K;
    const ResampleRows rows = wave_resample_rows(rs_lds_floats(C, K), C, K);
    float* const zl = rows.zl; float* const wraw = rows.wraw;
    const int lane = lane_id();
    // All global inputs of a ray (direction, depths or their uniforms, densities, the K inverse-CDF uniforms) are loaded ONE RAY
    // AHEAD into registers: the ray's own phases then never wait for HBM (three exposed round trips per ray before).
    struct RayIn { float dx, dy, dz, zv0, zv1, dens0, dens1, u0, u1, u2; };      // scalars only: indexed members end up in scratch
    const bool fits = C <= 128 && K <= 192;
    auto load_in = [&](int64_t n) -> RayIn {
        RayIn r;
        const float* dd = a.dirs + n * a.dirs_stride;
        r.dx = dd[0]; r.dy = dd[1]; r.dz = dd[2];
        // Philox mode: lane j's one block of the ray carries u_strat(n, j) and u_inv(n, j + {0, 64, 128})   (device_common.h)
        Philox4 blk = {{0u, 0u, 0u, 0u}};
        const bool draw = !a.u_inv || (!a.z && !a.u_strat);
        if (draw) blk = philox_ray_block(a.rng_seed, n + a.rng_ray_offset, lane);
        auto depth_of = [&](int j, bool first) {
            if (a.z) return a.z[n * C + j];
            const float uu = a.u_strat ? a.u_strat[n * C + j] : (first ? u01_from_bits(blk.w[0]) : philox_u_strat(a.rng_seed, n + a.rng_ray_offset, j));
            return a.z_base[j] + uu * a.z_jitter;
        };
        r.zv0 = r.zv1 = r.dens0 = r.dens1 = 0.0f;
        if (lane < C) { r.zv0 = depth_of(lane, true); r.dens0 = a.density[n * C + lane]; }
        if (lane + 64 < C) { r.zv1 = depth_of(lane + 64, false); r.dens1 = a.density[n * C + lane + 64]; }
        if (a.u_inv) {
            const float* un = a.u_inv + n * K;
            r.u0 = (lane < K) ? un[lane] : 0.0f;
            r.u1 = (lane + 64 < K) ? un[lane + 64] : 0.0f;
            r.u2 = (lane + 128 < K) ? un[lane + 128] : 0.0f;
        } else {
            r.u0 = u01_from_bits(blk.w[1]); r.u1 = u01_from_bits(blk.w[2]); r.u2 = u01_from_bits(blk.w[3]);
        }
        return r;
    };
    const int64_t stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
    int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block();
    if (n >= a.N) return;
    RayIn cur = {};
    if (fits) cur = load_in(n);
    for (; n < a.N; n += stride) {
        RayIn nxt = cur;
        if (fits && n + stride < a.N) nxt = load_in(n + stride);
        lds_wave_sync();
        float nrm;
        if (fits) {
            nrm = norm3(cur.dx, cur.dy, cur.dz);
            if (lane < C) { zl[lane] = cur.zv0; if (a.z_coarse) a.z_coarse[n * C + lane] = cur.zv0; }
            if (lane + 64 < C) { zl[lane + 64] = cur.zv1; if (a.z_coarse) a.z_coarse[n * C + lane + 64] = cur.zv1; }
        } else {
            const float* dd = a.dirs + n * a.dirs_stride;
            nrm = norm3(dd[0], dd[1], dd[2]);
            for (int j = lane; j < C; j += 64) {
                const float zv = a.z ? a.z[n * C + j]
                                     : (a.z_base[j] + (a.u_strat ? a.u_strat[n * C + j] : philox_u_strat(a.rng_seed, n + a.rng_ray_offset, j)) * a.z_jitter);
                zl[j] = zv;
                if (a.z_coarse) a.z_coarse[n * C + j] = zv;
            }
        }
        lds_wave_sync();
        const float* sg = a.density + n * C;
        const int soft = a.softplus;
        const float dens0 = cur.dens0, dens1 = cur.dens1, cu0 = cur.u0, cu1 = cur.u1, cu2 = cur.u2;   // by-value captures: a reference to `cur` pins it in scratch
        wave_sigma_to_weights(C, NERF_AMD_ACT_RELU,
                              [=](int s) { const float d = fits ? ((s >> 6) ? dens1 : dens0) : sg[s]; return soft ? softplus_f(d) : d; },
                              [=](int s) { return zl[s] * nrm; },
                              [=](int s, float wv, float) { wraw[s] = wv; });
        lds_wave_sync();
        wave_blur_pdf(wraw, C, a.alpha, rows.pw, a.w_prop ? a.w_prop + n * C : nullptr);
        wave_midpoints(zl, C, rows.bins);                                      // mid-points of the RAW depths
        lds_wave_sync();
        const float* un = a.u_inv ? a.u_inv + n * K : nullptr;
        const uint64_t seed = a.rng_seed; const int64_t nn = n + a.rng_ray_offset;
        wave_inverse_sample(rows, C - 2,
                            [=](int i, int k) {
                                if (fits) return i == 0 ? cu0 : (i == 1 ? cu1 : cu2);
                                if (un) return un[k];
                                return philox_u_inv(seed, nn, k);                                  // generic shapes
                            },
                            K, 1, a.z_fine + n * K, a.below ? a.below + n * K : nullptr, nullptr);
        cur = nxt;
    }
}

// ------------------------------------------------------------------------------------------------
// Disparity ray spacing (Mip-NeRF 360, Barron et al. 2022, section 3 / eq. 11-13 with g(x) = 1/x; not in the reference -- the build's
// own definition).  Samples are drawn and resampled in the normalised distance s in [0, 1], uniform in disparity:
//   W(s)    = 1 / ((1 - sb) gn + sb gf),  sb = clamp(s, 0, 1)       gn = fp32(1/near), gf = fp32(1/far) (rounded once on the host)
//   W^-1(z) = (1/zb - gn) / (gf - gn),    zb = clamp(z, near, far)
// every operation a separate fp32 rounding in exactly this order (-ffp-contract=off), IEEE division.  None of the linear-spacing
// kernels above reads any of this.
// ------------------------------------------------------------------------------------------------
struct WarpConsts { float near, far, gn, gf; };
DEVINL float warp_s_to_z(float s, const WarpConsts& c) {
    const float sb = fminf(fmaxf(s, 0.0f), 1.0f);
    return 1.0f / ((1.0f - sb) * c.gn + sb * c.gf);
}
DEVINL float warp_z_to_s(float z, const WarpConsts& c) {
    const float zb = fminf(fmaxf(z, c.near), c.far);
    return (1.0f / zb - c.gn) / (c.gf - c.gn);
}

// elementwise s -> z = W(s) (inverse: z -> s) over (N,S), optionally pts (N,S,3) = o + z d (point_on_ray, as in stratified_points_kernel)
__global__ void warp_depths_kernel(const float* __restrict__ in, const float* __restrict__ rays, int64_t N, int S, int inverse, WarpConsts c,
                                   float* __restrict__ out, float* __restrict__ pts) {
    const int64_t total = N * S;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const float zv = inverse ? warp_z_to_s(in[i], c) : warp_s_to_z(in[i], c);
        out[i] = zv;
        if (pts) point_on_ray(rays + (i / S) * 6, zv, pts + i * 3);
    }
}

// the coarse draw in s: s_j = (float)j r + u r with r = fp32(1/C) -- sampler_samples' expression at near = 0, res = 1/C -- then
// z = W(s) and pts = o + z d (point_on_ray).  u: explicit (N,C), or word 0 of the 'RS' Philox block of global ray n + ray_offset (philox_u_strat).
__global__ void warped_stratified_kernel(const float* __restrict__ rays, const float* __restrict__ u, int64_t N, int C, float res, uint64_t seed,
                                         int64_t ray_offset, WarpConsts c, float* __restrict__ s_out, float* __restrict__ z_out,
                                         float* __restrict__ pts) {
    const int64_t total = N * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / C;
        const int j = (int)(i - n * C);
        const float uu = u ? u[i] : philox_u_strat(seed, n + ray_offset, j);
        const float sv = (float)j * res + uu * res;
        const float zv = warp_s_to_z(sv, c);
        s_out[i] = sv;
        z_out[i] = zv;
        if (pts) point_on_ray(rays + n * 6, zv, pts + i * 3);
    }
}

// the tail of the two warped fused kernels: the sorted s_fine row sf[K] (LDS) -> s_fine (optional) and z_fine = W(s_fine)
DEVINL void wave_unwarp_samples(const float* sf, int K, const WarpConsts& c, float* s_fine, float* z_fine) {
    for (int k = lane_id(); k < K; k += 64) {
        const float sv = sf[k];
        if (s_fine) s_fine[k] = sv;
        z_fine[k] = warp_s_to_z(sv, c);
    }
}

// The fused per-ray step between the two MLP kernels under disparity spacing: weights from the METRIC depths W(s_c) |d|, max-blur,
// inverse sampling over the mid-points of s_c, then z_fine = W(s_fine).  One wavefront per ray.  Its stages are resample_kernel's:
// wave_sigma_to_weights, wave_blur_pdf, wave_midpoints (of s_c instead of z) and wave_inverse_sample on the rows of resample_rows; its
// tail, wave_unwarp_samples, is the windowed warped kernel's.  A kernel of its own so that resample_kernel's register budget and occupancy
// stay as they are.
struct WarpedResampleArgs {
    const float* density; const float* s_c; const float* dirs; int dirs_stride; const float* u_inv; int64_t N; int C; int K; int softplus;
    float alpha; WarpConsts c; float* z_fine; float* s_fine; int64_t* below; float* w_prop; uint64_t rng_seed; int64_t rng_ray_offset;
};

__global__ __launch_bounds__(256) void warped_resample_kernel(WarpedResampleArgs a) {
    const int C = a.C, K = a.K;
    const ResampleRows rows = wave_resample_rows(warped_lds_floats(C, K), C, K);
    float* const zl = rows.zl; float* const wraw = rows.wraw;
    float* const sf = rows.tail; float* const uu = sf + K;
    const int lane = lane_id();
    const WarpConsts c = a.c;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < a.N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        const float* dd = a.dirs + n * a.dirs_stride;
        const float nrm = norm3(dd[0], dd[1], dd[2]);
        const float* sc = a.s_c + n * C;
        for (int j = lane; j < C; j += 64) zl[j] = warp_s_to_z(sc[j], c);
        const int64_t nn = n + a.rng_ray_offset;
        for (int k = lane; k < K; k += 64) uu[k] = a.u_inv ? a.u_inv[n * K + k] : philox_u_inv(a.rng_seed, nn, k);   // words 1..3 of the 'RS' blocks
        lds_wave_sync();
        const float* sg = a.density + n * C;
        const int soft = a.softplus;
        wave_sigma_to_weights(C, NERF_AMD_ACT_RELU,
                              [=](int s) { const float d = sg[s]; return soft ? softplus_f(d) : d; },
                              [=](int s) { return zl[s] * nrm; },
                              [=](int s, float wv, float) { wraw[s] = wv; });
        lds_wave_sync();
        wave_blur_pdf(wraw, C, a.alpha, rows.pw, a.w_prop ? a.w_prop + n * C : nullptr);
        wave_midpoints(sc, C, rows.bins);                                      // mid-points of s_c
        lds_wave_sync();
        wave_inverse_sample(rows, C - 2, [=](int, int k) { return uu[k]; }, K, 1, sf, a.below ? a.below + n * K : nullptr, nullptr);
        lds_wave_sync();
        wave_unwarp_samples(sf, K, c, a.s_fine ? a.s_fine + n * K : nullptr, a.z_fine + n * K);
    }
}

// ------------------------------------------------------------------------------------------------
// The second proposal round (Mip-NeRF 360): the fused resampling step on EXPLICIT sorted coordinates -- the first round's output -- with
// the K inverse-CDF uniforms of columns u_col0 .. u_col0 + K - 1 of the ray's Philox stream instead of its first K (the two-round stream
// has prop_pnum + n_fine + 1 columns; the fine resampling reads behind the first prop_pnum).
// ------------------------------------------------------------------------------------------------
// uu[k] = philox_u_inv(seed, nn, u_col0 + k) for k < K.  One wavefront; lane j runs only those of its own blocks 64 b + j that carry a
// column of the window -- a block holds columns 192 b + j + {0, 64, 128} in words 1..3 (device_common.h) -- so the window costs about
// K / 192 + 1 blocks per lane where philox_u_inv per column would cost K / 64.
DEVINL void wave_window_uniforms(float* uu, uint64_t seed, int64_t nn, int u_col0, int K) {
    const int lane = lane_id();
    for (int b = u_col0 / 192; 192 * b < u_col0 + K; ++b) {
        const int k0 = 192 * b + lane - u_col0;                                // window index of the block's word 1
        const bool in0 = k0 >= 0 && k0 < K, in1 = k0 + 64 >= 0 && k0 + 64 < K, in2 = k0 + 128 >= 0 && k0 + 128 < K;
        if (!(in0 || in1 || in2)) continue;
        const Philox4 p = philox_ray_block(seed, nn, 64 * b + lane);
        if (in0) uu[k0] = u01_from_bits(p.w[1]);
        if (in1) uu[k0 + 64] = u01_from_bits(p.w[2]);
        if (in2) uu[k0 + 128] = u01_from_bits(p.w[3]);
    }
}

// resample_kernel (WARPED = false: x = metric depths z) and warped_resample_kernel (WARPED = true: x = s, weights from W(s) |d|, bins in s,
// z_fine = W(s_fine)) behind the window: wave_sigma_to_weights, wave_blur_pdf's loop (a copy, for the measured reason given at it),
// wave_midpoints and wave_inverse_sample (and, WARPED, wave_unwarp_samples) in the one-round kernels' order, so a round-two call equals
// the single-stage call given the same columns as a tensor.  resample_kernel binds lane j to ONE Philox block, which holds only at
// u_col0 = 0; here a lane's samples come from other blocks, so the uniforms go through an LDS row and only the ray's global loads --
// direction, coordinates, densities -- stay one ray ahead in registers (C <= 128).  Kernels of their own: the one-round kernels'
// register budget and occupancy stay as they are.
struct ResampleWindowArgs {
    const float* density; const float* x; const float* dirs; int dirs_stride; int64_t N; int C; int K; int u_col0; float alpha; WarpConsts c;
    float* z_fine; float* s_fine; uint64_t rng_seed; int64_t rng_ray_offset;
};

template <bool WARPED>
__global__ __launch_bounds__(256) void resample_window_kernel(ResampleWindowArgs a) {
    const int C = a.C, K = a.K;
    const ResampleRows rows = wave_resample_rows(rsw_lds_floats(C, K, WARPED), C, K);
    float* const zl = rows.zl; float* const wraw = rows.wraw;
    float* const uu = rows.tail; float* const sf = uu + K;                       // (sf: WARPED only)
    float* const xl = WARPED ? rows.cdf : zl;                                    // the bin coordinates: s parks in the cdf row, free until the inverse sampling writes it
    const int lane = lane_id();
    const WarpConsts c = a.c;
    struct RayIn { float dx, dy, dz, x0, x1, dens0, dens1; };                    // scalars only: indexed members end up in scratch
    const bool fits = C <= 128;
    auto load_in = [&](int64_t n) -> RayIn {
        RayIn r;
        const float* dd = a.dirs + n * a.dirs_stride;
        r.dx = dd[0]; r.dy = dd[1]; r.dz = dd[2];
        r.x0 = r.x1 = r.dens0 = r.dens1 = 0.0f;
        if (lane < C) { r.x0 = a.x[n * C + lane]; r.dens0 = a.density[n * C + lane]; }
        if (lane + 64 < C) { r.x1 = a.x[n * C + lane + 64]; r.dens1 = a.density[n * C + lane + 64]; }
        return r;
    };
    const int64_t stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
    int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block();
    if (n >= a.N) return;
    RayIn cur = {};
    if (fits) cur = load_in(n);
    for (; n < a.N; n += stride) {
        RayIn nxt = cur;
        if (fits && n + stride < a.N) nxt = load_in(n + stride);
        lds_wave_sync();
        float nrm;
        if (fits) {
            nrm = norm3(cur.dx, cur.dy, cur.dz);
            if (lane < C) { zl[lane] = WARPED ? warp_s_to_z(cur.x0, c) : cur.x0; if (WARPED) xl[lane] = cur.x0; }
            if (lane + 64 < C) { zl[lane + 64] = WARPED ? warp_s_to_z(cur.x1, c) : cur.x1; if (WARPED) xl[lane + 64] = cur.x1; }
        } else {
            const float* dd = a.dirs + n * a.dirs_stride;
            nrm = norm3(dd[0], dd[1], dd[2]);
            for (int j = lane; j < C; j += 64) {
                const float xv = a.x[n * C + j];
                zl[j] = WARPED ? warp_s_to_z(xv, c) : xv;
                if (WARPED) xl[j] = xv;
            }
        }
        wave_window_uniforms(uu, a.rng_seed, n + a.rng_ray_offset, a.u_col0, K);
        lds_wave_sync();
        const float* sg = a.density + n * C;
        const float dens0 = cur.dens0, dens1 = cur.dens1;                        // by-value captures: a reference to `cur` pins it in scratch
        wave_sigma_to_weights(C, NERF_AMD_ACT_RELU,
                              [=](int s) { return fits ? ((s >> 6) ? dens1 : dens0) : sg[s]; },
                              [=](int s) { return zl[s] * nrm; },
                              [=](int s, float wv, float) { wraw[s] = wv; });
        lds_wave_sync();
        // wave_blur_pdf's loop without w_prop, kept as a copy: through the call this kernel takes 2 more VGPRs and, per 640 000 rays,
        // 1194.5 us against 1177.0 us (<false>) and 1334.9 us against 1314.1 us (<true>), outside the spread of 12.0 / 7.0 us
        for (int j = lane; j < C; j += 64) {
            const float cw = wraw[j];
            const float front = (j == 0) ? cw : fmaxf(wraw[j - 1], cw);
            const float rear = (j == C - 1) ? cw : fmaxf(cw, wraw[j + 1]);
            if (j >= 1 && j <= C - 2) rows.pw[j - 1] = 0.5f * (front + rear) + a.alpha;   // pdf over weights[1:-1]
        }
        wave_midpoints(xl, C, rows.bins);                                        // mid-points of the coordinates
        lds_wave_sync();
        float* out = a.z_fine + n * K;
        wave_inverse_sample(rows, C - 2, [=](int, int k) { return uu[k]; }, K, 1, WARPED ? sf : out, nullptr, nullptr);
        if (WARPED) {
            lds_wave_sync();
            wave_unwarp_samples(sf, K, c, a.s_fine ? a.s_fine + n * K : nullptr, out);
        }
        cur = nxt;
    }
}

// ---------------------------------------------------------------------------------------- row 10
struct CompositeArgs {
    const float* rgbo; const float* z; int z_stride; const float* dirs; int dirs_stride; int64_t N; int S;
    int flags; int act; float sigma_shift; float near, far; const float* normal; const float* cam_dir;
    float* rgb; float* weights; float* depth; float* normal_img;
};

// Fast path of the compositing kernel for S <= 64 NCH (NCH = 2 or 4) without normals (the render path): a ray is NCH 64-lane chunks;
// all of its loads (one 16-byte rgbo record and one z per lane and chunk) are issued up front -- the neighbour z of the transmittance
// step comes from a lane shuffle instead of a second load -- and the NEXT ray of this wavefront is loaded before the current
// one is reduced, so two rays' worth of HBM requests are in flight per wave.  Same arithmetic, same order as the generic path.
template <int NCH>
struct RayRecs { f32x4 c[NCH]; float z[NCH]; float dx, dy, dz; };
// ROWS (the empty-ray skip, nerf_amd_render with skip_min_optical_depth > 0): the rgbo (and normal) rows are COMPACT -- ray n's row is
// rows[n], -1 for a ray the fine network was not run on, which reads an all-zero row; depths, directions and every output stay indexed
// by n.  Without ROWS nothing of this is compiled in.
template <int NCH, bool ROWS>
DEVINL RayRecs<NCH> load_ray(const CompositeArgs& a, const int32_t* rows, int64_t n, int lane) {
    RayRecs<NCH> r;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t row = n;
    if (ROWS) row = rows[n];
    const bool live = !ROWS || row >= 0;
    const f32x4* px = reinterpret_cast<const f32x4*>(a.rgbo) + row * a.S;
    const float* zz = a.z + n * a.z_stride;
    const float* dd = a.dirs + n * a.dirs_stride;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int s = 64 * k + lane;
        r.c[k] = (s < a.S && live) ? px[s] : zero;
        r.z[k] = (s < a.S) ? zz[s] : 0.0f;
    }
    r.dx = dd[0]; r.dy = dd[1]; r.dz = dd[2];
    return r;
}
template <int NCH>
DEVINL void composite_ray_fast(const CompositeArgs& a, int64_t n, const RayRecs<NCH>& r, int lane) {
    const int S = a.S;
    const bool mul = (a.flags & 1) != 0;
    const float nrm = mul ? norm3(r.dx, r.dy, r.dz) : 1.0f;
    float zn[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) zn[k] = mul ? r.z[k] * nrm : r.z[k];
    float accr = 0.0f, accg = 0.0f, accb = 0.0f, accw = 0.0f, accd = 0.0f;
    double carry = 1.0;
    float* wout = a.weights ? a.weights + n * S : nullptr;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (k > 0 && 64 * k >= S) break;                        // wave-uniform
        const int s = 64 * k + lane;
        float nx = __shfl_down(zn[k], 1, 64);                   // z of sample s + 1: the next lane, or lane 0 of the next chunk
        if (k + 1 < NCH) { const float first = __shfl(zn[k + 1 < NCH ? k + 1 : k], 0, 64); if (lane == 63) nx = first; }
        float w = 0.0f;
        double p = 1.0;
        if (s < S) {
            const float delta = (s + 1 < S) ? (nx - zn[k]) : 1e10f;
            const float m = expf(-density_act(r.c[k][3] + a.sigma_shift, a.act) * delta);
            w = 1.0f - m; p = (double)(m + 1e-10f);
        }
        const double incl = wave_incl_scan_mul(p);
        const double excl = wave_shift_up1(incl, 1.0);
        w *= (float)(carry * excl);
        carry *= wave_last(incl);
        if (s < S) {
            accr += w * r.c[k][0]; accg += w * r.c[k][1]; accb += w * r.c[k][2]; accw += w; accd += w * zn[k];
            if (wout) wout[s] = w;
        }
    }
    accr = wave_sum(accr); accg = wave_sum(accg); accb = wave_sum(accb); accw = wave_sum(accw); accd = wave_sum(accd);
    if (lane == 0) {
        if (a.flags & 2) { const float bg = 1.0f - accw; accr += bg; accg += bg; accb += bg; }
        a.rgb[n * 3] = accr; a.rgb[n * 3 + 1] = accg; a.rgb[n * 3 + 2] = accb;
        if (a.depth) a.depth[n] = (accd - a.near) / (a.far - a.near);
    }
}
template <int NCH, bool ROWS>
DEVINL void composite_rays_fast(const CompositeArgs& a, const int32_t* rows, int lane) {
    const int64_t stride = (int64_t)gridDim.x * WAVES_PER_BLOCK;
    int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block();
    if (n >= a.N) return;
    RayRecs<NCH> cur = load_ray<NCH, ROWS>(a, rows, n, lane);
    for (; n < a.N; n += stride) {
        RayRecs<NCH> nxt = cur;
        if (n + stride < a.N) nxt = load_ray<NCH, ROWS>(a, rows, n + stride, lane);
        composite_ray_fast<NCH>(a, n, cur, lane);
        cur = nxt;
    }
}

template <bool ROWS>
DEVINL void composite_rays(const CompositeArgs& a, const int32_t* rows) {
    const int S = a.S;
    const int lane = lane_id();
    if (S <= 256 && a.normal == nullptr && a.normal_img == nullptr) {
        if (S <= 128) composite_rays_fast<2, ROWS>(a, rows, lane);
        else composite_rays_fast<4, ROWS>(a, rows, lane);
        return;
    }
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < a.N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        const float* dd = a.dirs + n * a.dirs_stride;
        const bool mul = (a.flags & 1) != 0;
        const float nrm = mul ? norm3(dd[0], dd[1], dd[2]) : 1.0f;
        const float* zz = a.z + n * a.z_stride;
        int64_t row = n;
        if (ROWS) row = rows[n];
        const bool live = !ROWS || row >= 0;                        // (ROWS: a ray without a row composites zeros)
        const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
        const f32x4* px = reinterpret_cast<const f32x4*>(a.rgbo) + row * S;
        float accr = 0.0f, accg = 0.0f, accb = 0.0f, accw = 0.0f, accd = 0.0f, accn = 0.0f;
        float cx = 0.0f, cy = 0.0f, cz = 0.0f;
        if (a.normal_img) { cx = a.cam_dir[0]; cy = a.cam_dir[1]; cz = a.cam_dir[2]; }
        float* wout = a.weights ? a.weights + n * S : nullptr;
        const float* nm = a.normal ? a.normal + row * S * 3 : nullptr;
        const float shift = a.sigma_shift;
        wave_sigma_to_weights(S, a.act, [&](int s) { return (live ? px[s][3] : 0.0f) + shift; },
                              [&](int s) { return mul ? zz[s] * nrm : zz[s]; },
                              [&](int s, float w, float zn) {
                                  const f32x4 c = live ? px[s] : zero;
                                  accr += w * c[0]; accg += w * c[1]; accb += w * c[2];
                                  accw += w; accd += w * zn;
                                  if (nm) {
                                      const float n0 = live ? nm[s * 3] : 0.0f, n1 = live ? nm[s * 3 + 1] : 0.0f, n2 = live ? nm[s * 3 + 2] : 0.0f;
                                      accn += w * ((n0 * cx + n1 * cy) + n2 * cz);
                                  }
                                  if (wout) wout[s] = w;
                              });
        accr = wave_sum(accr); accg = wave_sum(accg); accb = wave_sum(accb); accw = wave_sum(accw);
        accd = wave_sum(accd);
        if (a.normal_img) accn = wave_sum(accn);
        if (lane == 0) {
            if (a.flags & 2) { const float bg = 1.0f - accw; accr += bg; accg += bg; accb += bg; }
            a.rgb[n * 3] = accr; a.rgb[n * 3 + 1] = accg; a.rgb[n * 3 + 2] = accb;
            if (a.depth) a.depth[n] = (accd - a.near) / (a.far - a.near);
            if (a.normal_img) a.normal_img[n] = (accn + 1.0f) * 0.5f;
        }
    }
}
__global__ __launch_bounds__(256) void composite_kernel(CompositeArgs a) { composite_rays<false>(a, nullptr); }
__global__ __launch_bounds__(256) void composite_rows_kernel(CompositeArgs a, const int32_t* __restrict__ rows) { composite_rays<true>(a, rows); }

// ---------------------------------------------------------------------------------------- empty-ray skip (include/nerf_amd.h: nerf_amd_ray_alive)
// The optical depth D of the proposal histogram of one ray, one wavefront per ray, any C >= 2: every term is formed in fp64 from the fp32
// inputs, the lanes' partial sums meet in an fp64 butterfly (no LDS, no atomics).  max(sigma, 0) is written as a select that keeps a NaN:
// D is then NaN, D < D_min is false and the ray stays alive.  flags[n] = !(D < D_min).
struct RayAliveArgs { const float* density; const float* z; int z_stride; const float* dirs; int dirs_stride; int64_t N; int C; double d_min; uint8_t* flags; };
__global__ __launch_bounds__(256) void ray_alive_kernel(RayAliveArgs a) {
    const int lane = lane_id();
    const int C = a.C;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < a.N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        const float* sg = a.density + n * C;
        const float* zz = a.z + n * a.z_stride;
        double acc = 0.0;
        for (int s = lane; s < C - 1; s += 64) {
            const float sv = sg[s];
            const double sig = sv < 0.0f ? 0.0 : (double)sv;
            acc += sig * ((double)zz[s + 1] - (double)zz[s]);
        }
        acc = wave_sum_d(acc);
        if (lane == 0) {
            const float* dd = a.dirs + n * a.dirs_stride;
            const double dx = dd[0], dy = dd[1], dz = dd[2];
            const float sl = sg[C - 1];
            const double closing = (sl < 0.0f ? 0.0 : (double)sl) * 1e10;       // the last delta: 1e10, not scaled by |d|
            const double D = sqrt((dx * dx + dy * dy) + dz * dz) * acc + closing;
            a.flags[n] = !(D < a.d_min) ? 1 : 0;
        }
    }
}
// Ordered stream compaction of the flags in tiles of 256 (one per workgroup): a ballot + popcount per wave, the four wave counts through
// LDS -> one count per tile; ONE workgroup turns the tile counts into exclusive offsets (wave scan + carry, 256 tiles per step) and stores
// the total; the tiles then rank their alive rays -- offset of the tile + alive rays of the waves before + alive lanes below -- and write both
// tables.  Alive rays keep their order; no atomics: the result is a pure function of the flags.
constexpr int ALIVE_TILE = 256;
DEVINL unsigned long long alive_ballot(const uint8_t* flags, int64_t N, int64_t n, int* wave_count) {
    const unsigned long long m = __ballot(n < N && flags[n] != 0);
    if (lane_id() == 0) wave_count[wave_in_block()] = __popcll(m);
    __syncthreads();
    return m;
}
__global__ __launch_bounds__(256) void alive_count_kernel(const uint8_t* __restrict__ flags, int64_t N, int* __restrict__ tile_count) {
    __shared__ int wave_count[WAVES_PER_BLOCK];
    alive_ballot(flags, N, blockIdx.x * (int64_t)ALIVE_TILE + threadIdx.x, wave_count);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}
__global__ __launch_bounds__(256) void alive_offsets_kernel(int* __restrict__ tiles, int64_t n_tiles, int64_t* __restrict__ count) {
    __shared__ int wave_total[WAVES_PER_BLOCK];
    const int lane = lane_id(), wv = wave_in_block();
    int carry = 0;
    for (int64_t base = 0; base < n_tiles; base += 256) {
        const int64_t i = base + threadIdx.x;
        const int v = i < n_tiles ? tiles[i] : 0;
        const int incl = wave_incl_scan_add(v);
        if (lane == 63) wave_total[wv] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < WAVES_PER_BLOCK; ++k) { before += k < wv ? wave_total[k] : 0; total += wave_total[k]; }
        if (i < n_tiles) tiles[i] = carry + before + (incl - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = carry;
}
__global__ __launch_bounds__(256) void alive_tables_kernel(const uint8_t* __restrict__ flags, int64_t N, const int* __restrict__ tile_offset,
                                                           int32_t* __restrict__ row_of_ray, int64_t* __restrict__ ray_of_row) {
    __shared__ int wave_count[WAVES_PER_BLOCK];
    const int64_t n = blockIdx.x * (int64_t)ALIVE_TILE + threadIdx.x;
    const unsigned long long m = alive_ballot(flags, N, n, wave_count);
    if (n >= N) return;
    const int lane = lane_id(), wv = wave_in_block();
    int rank = tile_offset[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wv; ++k) rank += wave_count[k];
    const bool alive = (m >> lane) & 1ull;
    row_of_ray[n] = alive ? rank : -1;
    if (alive) ray_of_row[rank] = n;
}
// dst (n_rows, cols) = the rows ray_of_row[0 .. n_rows) of src (row stride src_stride floats)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, int64_t src_stride, const int64_t* __restrict__ ray_of_row, int64_t n_rows,
                                                          int cols, float* __restrict__ dst) {
    const int64_t total = n_rows * cols;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols;
        dst[i] = src[ray_of_row[r] * src_stride + (i - r * cols)];
    }
}

// ---------------------------------------------------------------------------------------- depth quantiles and opacity of a composited ray
// The definition is in include/nerf_amd.h (nerf_amd_ray_depth_stats) and, in fp64, in tests/depth_stats_ref.py.  One wavefront per ray, a
// ray in 64-sample chunks: the cumulative mass C is an fp64 wave scan plus an fp64 carry, a ballot of C_incl >= q picks the crossing lane,
// which interpolates in fp64 and stores; t_{k+1} is the next lane's t, or lane 0 of the next chunk (loaded one chunk ahead).  All quantiles
// are resolved in the one pass.  No LDS, no atomics, no host state: deterministic and capturable; no limit on S.
struct DepthStatsArgs {
    const float* w; const float* z; int z_stride; int closed; const float* dirs; int dirs_stride; int64_t N; int S; int mul_norm;
    float q[NERF_AMD_DEPTH_QUANTILES_MAX]; int nq; float near, far; float* opacity; float* depth_q;
};
__global__ __launch_bounds__(256) void ray_depth_stats_kernel(DepthStatsArgs a) {
    const int lane = lane_id();
    const int S = a.S, E = a.S + (a.closed ? 1 : 0);
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < a.N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        float nrm = 1.0f;
        if (a.mul_norm) { const float* dd = a.dirs + n * a.dirs_stride; nrm = norm3(dd[0], dd[1], dd[2]); }
        const float* ww = a.w + n * S;
        const float* zz = a.z + n * a.z_stride;
        float* dq = a.depth_q ? a.depth_q + n * a.nq : nullptr;
        const float scale = a.far - a.near;
        double carry = 0.0;
        int open_q = dq ? (1 << a.nq) - 1 : 0;                  // bit j: quantile j has not crossed yet (wave-uniform)
        float z_nxt = (lane < E) ? zz[lane] : 0.0f;
        for (int base = 0; base < S; base += 64) {
            const int s = base + lane;
            const float wv = (s < S) ? ww[s] : 0.0f;
            const float t = a.mul_norm ? z_nxt * nrm : z_nxt;   // the arithmetic of composite_kernel's zn
            z_nxt = (s + 64 < E) ? zz[s + 64] : 0.0f;
            float t_up = __shfl_down(t, 1, 64);                  // t of sample s + 1: the next lane, or lane 0 of the next chunk
            const float first = __shfl(a.mul_norm ? z_nxt * nrm : z_nxt, 0, 64);
            if (lane == 63) t_up = first;
            const double incl = wave_incl_scan_add((double)wv) + carry;
            const double excl = wave_shift_up1(incl, carry);
            carry = wave_last(incl);
#pragma unroll
            for (int j = 0; j < NERF_AMD_DEPTH_QUANTILES_MAX; ++j) {
                if (!(open_q & (1 << j))) continue;             // wave-uniform
                const double q = (double)a.q[j];
                // (w > 0 holds at the crossing by definition; asked for here so that the last bit of a prefix never selects an empty interval)
                const unsigned long long hit = __ballot(s < S && wv > 0.0f && incl >= q);
                if (!hit) continue;
                open_q &= ~(1 << j);
                if (lane == __builtin_ctzll(hit)) {
                    float D = t;                                 // k = S - 1 of an open row: no edge behind it
                    if (s + 1 < E) D = (float)((double)t + ((q - excl) / (double)wv) * ((double)t_up - (double)t));
                    dq[j] = (D - a.near) / scale;
                }
            }
        }
        if (lane == 0) {
            if (a.opacity) a.opacity[n] = (float)carry;
            if (open_q) {                                        // the ray never accumulates q: the far edge
                const float zl = zz[E - 1];
                const float D = a.mul_norm ? zl * nrm : zl;
                for (int j = 0; j < a.nq; ++j)
                    if (open_q & (1 << j)) dq[j] = (D - a.near) / scale;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- row 11
template <class T> static inline __host__ __device__ T gb_lds_floats(T C) { return C + 1; }               // per wave: the summed-area row sat[C + 1]
__global__ __launch_bounds__(256) void get_bounds_kernel(const float* __restrict__ w, const int64_t* __restrict__ below,
                                                        int64_t N, int C, int K, float* __restrict__ bounds) {
    float* sat = reinterpret_cast<float*>(smem) + wave_in_block() * gb_lds_floats(C);
    const int lane = lane_id();
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        double carry = 0.0;
        if (lane == 0) sat[0] = 0.0f;
        for (int base = 0; base < C; base += 64) {
            const int j = base + lane;
            const double p = (j < C) ? (double)w[n * C + j] : 0.0;
            const double incl = wave_incl_scan_add(p);
            if (j < C) sat[1 + j] = (float)(carry + incl);
            carry += wave_last(incl);
        }
        lds_wave_sync();
        const int64_t* bl = below + n * K;
        for (int k = lane; k < K - 1; k += 64) {
            const int st = (int)bl[k], en = (int)bl[k + 1] + 1;
            bounds[n * (K - 1) + k] = sat[en] - sat[st];
        }
    }
}

// ================================================================================================
// Backward kernels of the sampling / compositing rows: one wavefront per ray, the transmittance
// product's adjoint is a suffix sum.  Up to 1 024 samples per ray (4 / 8 / 16 register chunks).
//   forward:  m_i = exp(-act(sigma_i + shift) * delta_i),  q_i = m_i + 1e-10,  T_i = prod_{j<i} q_j,  w_i = (1 - m_i) T_i
//   given G_i = dL/dw_i:   dL/dm_j = -G_j T_j + (sum_{i>j} G_i w_i) / q_j,   dL/dsigma_j = dL/dm_j * (-delta_j m_j) * act'(sigma_j + shift)
// ================================================================================================
// Rows of any length up to 1 024 samples (round 5: `-t --fine_sample_pnum 256` merges 320 samples per ray, nerf_base.py:91-113 has no limit):
// the kernel is instantiated for 4 / 8 / 16 register chunks of 64 samples (7 registers per chunk) and the launcher picks by S.
constexpr int BWD_MAX_CHUNKS = 16;
struct WeightsBwdArgs {
    const float* sigma; int sigma_stride;      // sigma of sample s of ray n at sigma[(n*S + s) * sigma_stride + sigma_off]
    int sigma_off;
    const float* z; int z_stride; const float* dirs; int dirs_stride; int64_t N; int S; int mul_norm; int act; float sigma_shift;
    // composite extras (rgbo != nullptr): colours come from rgbo[(n*S+s)*4 + 0..2]
    const float* rgbo; const float* d_rgb; const float* d_weights; const float* d_depth; int white_bkg; float near, far;
    float* d_sigma; int d_sigma_stride; int d_sigma_off; float* d_rgbo;
};
DEVINL float density_act_grad(float x, int act) {
    if (act == 0) return x > 0.0f ? 1.0f : 0.0f;
    if (act == 2) return x > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-x));
    return 1.0f;
}
template <int BWD_CHUNKS>
__global__ __launch_bounds__(256) void weights_backward_kernel(WeightsBwdArgs a) {
    const int S = a.S;
    const int lane = lane_id();
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < a.N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        float nrm = 1.0f;
        if (a.mul_norm && a.dirs) { const float* dd = a.dirs + n * a.dirs_stride; nrm = norm3(dd[0], dd[1], dd[2]); }
        const float* zz = a.z + n * a.z_stride;
        float dr = 0.0f, dg = 0.0f, db = 0.0f, dd_ = 0.0f;
        if (a.d_rgb) { dr = a.d_rgb[n * 3]; dg = a.d_rgb[n * 3 + 1]; db = a.d_rgb[n * 3 + 2]; }
        if (a.d_depth) dd_ = a.d_depth[n] / (a.far - a.near);
        const float bg = (a.white_bkg && a.d_rgb) ? ((dr + dg) + db) : 0.0f;       // rgb += 1 - sum w
        float m[BWD_CHUNKS], T[BWD_CHUNKS], G[BWD_CHUNKS], delta[BWD_CHUNKS], x[BWD_CHUNKS];
        double carry = 1.0, gw_carry = 0.0;
        double P[BWD_CHUNKS];                                                       // inclusive prefix of G_i w_i
#pragma unroll
        for (int c = 0; c < BWD_CHUNKS; ++c) {
            const int s = c * 64 + lane;
            const bool ok = s < S;
            m[c] = 1.0f; T[c] = 0.0f; G[c] = 0.0f; delta[c] = 0.0f; x[c] = 0.0f;
            double p = 1.0;
            float zn0 = 0.0f;
            if (c * 64 < S) {
                if (ok) {
                    zn0 = zz[s] * nrm;
                    delta[c] = (s + 1 < S) ? (zz[s + 1] * nrm - zn0) : 1e10f;
                    x[c] = a.sigma[(n * S + s) * a.sigma_stride + a.sigma_off] + a.sigma_shift;
                    m[c] = expf(-density_act(x[c], a.act) * delta[c]);
                    p = (double)(m[c] + 1e-10f);
                }
                const double incl = wave_incl_scan_mul(p);
                const double excl = wave_shift_up1(incl, 1.0);
                T[c] = (float)(carry * excl);
                carry *= wave_last(incl);
                float g = 0.0f;
                if (ok) {
                    if (a.d_weights) g += a.d_weights[n * S + s];
                    if (a.rgbo) {
                        const float* cc = a.rgbo + (n * S + s) * 4;
                        g += ((dr * cc[0] + dg * cc[1]) + db * cc[2]) - bg;
                    }
                    g += dd_ * zn0;
                }
                G[c] = g;
                const float w = (1.0f - m[c]) * T[c];
                const double gi = wave_incl_scan_add(ok ? (double)(g * w) : 0.0);
                P[c] = gw_carry + gi;
                gw_carry += wave_last(gi);
                if (ok && a.d_rgbo) {                                               // dL/dc_i = w_i * d_rgb
                    float* o = a.d_rgbo + (n * S + s) * 4;
                    o[0] = w * dr; o[1] = w * dg; o[2] = w * db;
                }
            }
        }
        const double total = gw_carry;
#pragma unroll
        for (int c = 0; c < BWD_CHUNKS; ++c) {
            const int s = c * 64 + lane;
            if (s < S) {
                const float suffix = (float)(total - P[c]);                         // sum_{i>s} G_i w_i
                const float dm = -G[c] * T[c] + suffix / (m[c] + 1e-10f);
                const float ds = dm * (-delta[c] * m[c]) * density_act_grad(x[c], a.act);
                a.d_sigma[(n * S + s) * a.d_sigma_stride + a.d_sigma_off] = ds;
            }
        }
    }
}

// maxBlurFilter backward (mip_methods.py:61-66): torch.maximum sends the gradient to the larger argument, half to each on a tie
__global__ void max_blur_backward_kernel(const float* __restrict__ w, const float* __restrict__ g, int64_t N, int S, float* __restrict__ dw) {
    const int64_t total = N * S;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = (int)(i % S);
        const float c = w[i];
        float acc = 0.0f;
        if (s == 0) acc += 0.5f * g[i];
        if (s == S - 1) acc += 0.5f * g[i];
        if (s + 1 < S) {                                    // mx_s = max(w_s, w_{s+1}) feeds rear_s and front_{s+1}
            const float o = w[i + 1];
            const float share = c > o ? 1.0f : (c == o ? 0.5f : 0.0f);
            acc += share * (0.5f * g[i] + 0.5f * g[i + 1]);
        }
        if (s >= 1) {                                       // mx_{s-1} = max(w_{s-1}, w_s) feeds rear_{s-1} and front_s
            const float o = w[i - 1];
            const float share = c > o ? 1.0f : (c == o ? 0.5f : 0.0f);
            acc += share * (0.5f * g[i - 1] + 0.5f * g[i]);
        }
        dw[i] = acc;
    }
}

// getBounds backward (addtional.py:14-18): bounds_k = sat[below_{k+1} + 1] - sat[below_k] = +sum of w over [below_k, below_{k+1}] (or minus the
// sum over the gap when the indices are not ascending)  ->  dw_j = sum_k g_k * ([st_k <= j < en_k] - [en_k <= j < st_k]).
// Every lane gathers its own j in ascending k: no atomics, reproducible.
template <class T> static inline __host__ __device__ T gbb_lds_words(T K) { return 2 * K; }               // per wave: below[K] (int) g[K]
__global__ __launch_bounds__(256) void get_bounds_backward_kernel(const int64_t* __restrict__ below, const float* __restrict__ g, int64_t N, int C,
                                                                  int K, float* __restrict__ dw) {
    int* bl_lds = reinterpret_cast<int*>(smem) + wave_in_block() * gbb_lds_words(K);
    float* g_lds = reinterpret_cast<float*>(bl_lds + K);
    const int lane = lane_id();
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        for (int k = lane; k < K; k += 64) {
            int b = (int)below[n * K + k];
            bl_lds[k] = b < 0 ? 0 : (b > C ? C : b);
            g_lds[k] = (k < K - 1) ? g[n * (K - 1) + k] : 0.0f;
        }
        lds_wave_sync();
        for (int j = lane; j < C; j += 64) {
            float acc = 0.0f;
            for (int k = 0; k < K - 1; ++k) {
                const int st = bl_lds[k];
                int en = bl_lds[k + 1] + 1;
                en = en > C ? C : en;
                if (j >= st && j < en) acc += g_lds[k];
                else if (j >= en && j < st) acc -= g_lds[k];
            }
            dw[n * C + j] = acc;
        }
    }
}

// Training dump (mlp_kernels.hip ActDump) -> row-major activations.  Block (subtile, K group) of the dump holds, for lane
// (h = lane >> 5, j = lane & 31), the 8 features 16 kg + 8 (e >> 2) + 4 h + (e & 3), e = 0..7, of sample 32 subtile + j
// (mlp_layout.h dmap_feature): two runs of four consecutive features.  ELEM = 2 (bf16) or 4 (fp32, halves 1 KiB apart).
static inline __host__ __device__ int frag_pitch(int n_kg, int elem) { return n_kg * 16 * elem + 16; }   // per wave: a 32-row tile, the row pitch padded by 16 bytes
static inline __host__ __device__ size_t frag_wave_bytes(int n_kg, int elem) { return (size_t)32 * frag_pitch(n_kg, elem); }
template <int ELEM>
__global__ __launch_bounds__(256) void frag_to_rows_kernel(const char* __restrict__ frag, int64_t n_sub, int n_kg, int64_t M,
                                                           char* __restrict__ out, int ld) {
    // One wavefront per subtile: the 32 x (16 n_kg) tile is transposed through LDS (row pitch padded by 16 bytes against bank
    // conflicts), so that the global side is 16-byte lane-linear on the way in AND on the way out (the subtile's 32 rows are one
    // contiguous block of the row-major matrix).
    const int lane = lane_id(), h = lane >> 5, j = lane & 31;
    constexpr int BLOCK = 512 * ELEM;                           // bytes per (subtile, K group)
    const int row_bytes = n_kg * 16 * ELEM;
    const int pitch = frag_pitch(n_kg, ELEM);
    char* tile = smem + (size_t)wave_in_block() * frag_wave_bytes(n_kg, ELEM);
    for (int64_t sub = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); sub < n_sub; sub += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        char* trow = tile + j * pitch;
        for (int kg = 0; kg < n_kg; ++kg) {
            const char* blk = frag + ((size_t)sub * 16 + kg) * BLOCK;
            if constexpr (ELEM == 2) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(blk + lane * 16);          // 8 bf16
                f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
                *reinterpret_cast<f32x2*>(trow + (16 * kg + 4 * h) * 2) = lo;
                *reinterpret_cast<f32x2*>(trow + (16 * kg + 8 + 4 * h) * 2) = hi;
            } else {
                *reinterpret_cast<f32x4*>(trow + (16 * kg + 4 * h) * 4) = *reinterpret_cast<const f32x4*>(blk + lane * 16);
                *reinterpret_cast<f32x4*>(trow + (16 * kg + 8 + 4 * h) * 4) = *reinterpret_cast<const f32x4*>(blk + 1024 + lane * 16);
            }
        }
        lds_wave_sync();
        const int chunks_per_row = row_bytes / 16;
        const int total = 32 * chunks_per_row;
        char* obase = out + (size_t)sub * 32 * ld * ELEM;
        for (int c = lane; c < total; c += 64) {
            const int r = c / chunks_per_row, q = c - r * chunks_per_row;
            if (sub * 32 + r < M)
                *reinterpret_cast<f32x4*>(obase + (size_t)r * ld * ELEM + q * 16) = *reinterpret_cast<const f32x4*>(tile + r * pitch + q * 16);
        }
    }
}

// frag_to_rows_kernel + relu_mask_bias_kernel in one pass over a layer: the subtile's activations go dump -> LDS -> row-major
// `act_out`, and while they sit in LDS the same 32 rows of `delta` (row-major, same shape) are masked in place by [act > 0] and
// summed per column.  Saves re-reading the activation matrix (4 instead of 5 matrix passes per layer).  Column sums: lane c owns
// 16-byte chunk c % cpr of rows c / cpr + (64 / cpr) i, i.e. a fixed set of columns; each wavefront writes ONE partial row of
// fp32 sums (deterministic, no atomics), `col_sum` has gridDim.x * WAVES_PER_BLOCK rows.
template <int ELEM>
__global__ __launch_bounds__(256) void frag_rows_mask_kernel(const char* __restrict__ frag, int64_t n_sub, int n_kg, int64_t M,
                                                             char* __restrict__ act_out, char* __restrict__ delta, float* __restrict__ col_sum) {
    const int lane = lane_id(), h = lane >> 5, j = lane & 31;
    constexpr int BLOCK = 512 * ELEM;
    constexpr int NV = 16 / ELEM;                                // values per 16-byte chunk
    const int row_bytes = n_kg * 16 * ELEM;
    const int pitch = frag_pitch(n_kg, ELEM);
    const int ld = n_kg * 16;
    char* tile = smem + (size_t)wave_in_block() * frag_wave_bytes(n_kg, ELEM);
    const int cpr = row_bytes / 16;                              // 16, 32 or 64: divides the wave size
    const int q = lane % cpr, r0 = lane / cpr, rstep = 64 / cpr;
    float acc[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = 0.0f;
    for (int64_t sub = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); sub < n_sub; sub += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        char* trow = tile + j * pitch;
        for (int kg = 0; kg < n_kg; ++kg) {
            const char* blk = frag + ((size_t)sub * 16 + kg) * BLOCK;
            if constexpr (ELEM == 2) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(blk + lane * 16);
                f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
                *reinterpret_cast<f32x2*>(trow + (16 * kg + 4 * h) * 2) = lo;
                *reinterpret_cast<f32x2*>(trow + (16 * kg + 8 + 4 * h) * 2) = hi;
            } else {
                *reinterpret_cast<f32x4*>(trow + (16 * kg + 4 * h) * 4) = *reinterpret_cast<const f32x4*>(blk + lane * 16);
                *reinterpret_cast<f32x4*>(trow + (16 * kg + 8 + 4 * h) * 4) = *reinterpret_cast<const f32x4*>(blk + 1024 + lane * 16);
            }
        }
        lds_wave_sync();
        const size_t base = (size_t)sub * 32 * ld * ELEM;
        for (int r = r0; r < 32; r += rstep) {
            if (sub * 32 + r >= M) break;
            const size_t off = base + (size_t)r * ld * ELEM + q * 16;
            typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
            if constexpr (ELEM == 4) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(tile + r * pitch + q * 16);
                f32x4 d = *reinterpret_cast<const f32x4*>(delta + off);
                *reinterpret_cast<f32x4*>(act_out + off) = a;
#pragma unroll
                for (int e = 0; e < 4; ++e) { if (!(a[e] > 0.0f)) d[e] = 0.0f; acc[e] += d[e]; }
                *reinterpret_cast<f32x4*>(delta + off) = d;
            } else {
                const u32x4 a = *reinterpret_cast<const u32x4*>(tile + r * pitch + q * 16);
                const u32x4 d = *reinterpret_cast<const u32x4*>(delta + off);
                *reinterpret_cast<u32x4*>(act_out + off) = a;
                uint32_t w[4] = {d[0], d[1], d[2], d[3]};
                const uint32_t aw[4] = {a[0], a[1], a[2], a[3]};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t lo = aw[e] & 0xFFFFu, hi = aw[e] >> 16;
                    if (!(lo != 0u && lo < 0x8000u)) w[e] &= 0xFFFF0000u;
                    if (!(hi != 0u && hi < 0x8000u)) w[e] &= 0x0000FFFFu;
                    acc[2 * e] += __builtin_bit_cast(float, w[e] << 16);
                    acc[2 * e + 1] += __builtin_bit_cast(float, w[e] & 0xFFFF0000u);
                }
                const u32x4 o = {w[0], w[1], w[2], w[3]};
                *reinterpret_cast<u32x4*>(delta + off) = o;
            }
        }
    }
    // lanes with equal q (lane bits >= log2 cpr) hold sums of the same columns: fold them, then lanes 0 .. cpr-1 write the partial row
    for (int m = cpr; m < 64; m <<= 1) {
#pragma unroll
        for (int e = 0; e < NV; ++e) acc[e] += __shfl_xor(acc[e], m, 64);
    }
    if (lane < cpr) {
        float* prow = col_sum + ((size_t)blockIdx.x * WAVES_PER_BLOCK + wave_in_block()) * (size_t)ld + q * NV;
#pragma unroll
        for (int e = 0; e < NV; ++e) prow[e] = acc[e];
    }
}

// First-layer / skip-layer operand of the wgrad GEMMs: row m = [x | positional_encoding_L(x) | 0 pad] (nerf_helper.py:38-48 order:
// per octave k the three sines, then the three cosines), NCOL = 3 + 6 L rounded up to 8, as bf16 (ELEM 2) or fp32 (ELEM 4).
// `normalize` divides x by its norm first (the view direction of mip_model.py:52).  bf16 rows take octave 0 from sincosf and the
// higher octaves by angle doubling like the forward kernels (error <= 2^9 * 1e-7, far below a bf16 ulp); fp32 rows call sincosf
// per octave.
template <int L, int ELEM>
__global__ __launch_bounds__(256) void encode_rows_kernel(const float* __restrict__ x, int x_stride, int64_t M, int normalize,
                                                          char* __restrict__ out) {
    constexpr int NCOL = (3 + 6 * L + 7) / 8 * 8;
    for (int64_t m = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; m < M; m += (int64_t)gridDim.x * blockDim.x) {
        const float* px = x + m * x_stride;
        float c[3] = {px[0], px[1], px[2]};
        if (normalize) { const float n = norm3(c[0], c[1], c[2]); c[0] /= n; c[1] /= n; c[2] /= n; }
        float v[NCOL];
#pragma unroll
        for (int q = 0; q < NCOL; ++q) v[q] = 0.0f;
        float sv[3], cv[3];
#pragma unroll
        for (int k = 0; k < L; ++k) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (ELEM == 4 || k == 0) sincosf(c[i] * (float)(1 << k), &sv[i], &cv[i]);
                else { const float s2 = 2.0f * sv[i]; const float ns = s2 * cv[i]; cv[i] = __builtin_fmaf(-s2, sv[i], 1.0f); sv[i] = ns; }
                v[3 + 6 * k + i] = sv[i];
                v[3 + 6 * k + 3 + i] = cv[i];
            }
        }
        v[0] = c[0]; v[1] = c[1]; v[2] = c[2];
        char* o = out + (size_t)m * NCOL * ELEM;
        if constexpr (ELEM == 4) {
#pragma unroll
            for (int q = 0; q < NCOL; q += 4) { f32x4 w = {v[q], v[q + 1], v[q + 2], v[q + 3]}; *reinterpret_cast<f32x4*>(o + q * 4) = w; }
        } else {
#pragma unroll
            for (int q = 0; q < NCOL; q += 8) {
                uint32_t w[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t lo = __builtin_bit_cast(uint32_t, v[q + 2 * e]), hi = __builtin_bit_cast(uint32_t, v[q + 2 * e + 1]);
                    const uint32_t rl = (lo + 0x7fffu + ((lo >> 16) & 1u)) >> 16, rh = (hi + 0x7fffu + ((hi >> 16) & 1u)) >> 16;   // RNE (finite inputs)
                    w[e] = rl | (rh << 16);
                }
                f32x4 pk = {__builtin_bit_cast(float, w[0]), __builtin_bit_cast(float, w[1]), __builtin_bit_cast(float, w[2]), __builtin_bit_cast(float, w[3])};
                *reinterpret_cast<f32x4*>(o + q * 2) = pk;
            }
        }
    }
}

// delta[i] = act[i] > 0 ? delta[i] : 0 -- the ReLU adjoint of the dgrad chain, in place (ELEM = 2: bf16 pairs, 4: fp32)
template <int ELEM>
__global__ void relu_mask_kernel(uint32_t* __restrict__ delta, const uint32_t* __restrict__ act, int64_t n_words) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t a = act[i];
        uint32_t d = delta[i];
        if constexpr (ELEM == 4) {
            if (!(__builtin_bit_cast(float, a) > 0.0f)) d = 0u;
        } else {                                             // two bf16: positive <=> sign bit clear and not (+)zero
            const uint32_t lo = a & 0xFFFFu, hi = a >> 16;
            if (!(lo != 0u && lo < 0x8000u)) d &= 0xFFFF0000u;
            if (!(hi != 0u && hi < 0x8000u)) d &= 0x0000FFFFu;
        }
        delta[i] = d;
    }
}

// The same with the bias gradient fused in: partial column sums of the MASKED delta, one fp32 row per (block, row group) -- no atomics,
// so that the result is reproducible; the caller adds the partial rows up.
// Thread t of a 256-thread block owns 32-bit word (t % W) of rows (t / W), (t / W) + 256 / W, ...; W = words per row <= 256.
template <int ELEM>
__global__ __launch_bounds__(256) void relu_mask_bias_kernel(uint32_t* __restrict__ delta, const uint32_t* __restrict__ act, int64_t rows, int W,
                                                             float* __restrict__ col_sum) {
    const int wc = threadIdx.x % W, r0 = threadIdx.x / W, rpb = 256 / W;
    float s0 = 0.0f, s1 = 0.0f;
    for (int64_t r = (int64_t)blockIdx.x * rpb + r0; r < rows; r += (int64_t)gridDim.x * rpb) {
        const int64_t i = r * W + wc;
        const uint32_t a = act[i];
        uint32_t d = delta[i];
        if constexpr (ELEM == 4) {
            if (!(__builtin_bit_cast(float, a) > 0.0f)) d = 0u;
            s0 += __builtin_bit_cast(float, d);
        } else {
            const uint32_t lo = a & 0xFFFFu, hi = a >> 16;
            if (!(lo != 0u && lo < 0x8000u)) d &= 0xFFFF0000u;
            if (!(hi != 0u && hi < 0x8000u)) d &= 0x0000FFFFu;
            s0 += __builtin_bit_cast(float, d << 16);           // bf16 -> fp32: the same bits in the upper half
            s1 += __builtin_bit_cast(float, d & 0xFFFF0000u);
        }
        delta[i] = d;
    }
    // deterministic: every (block, row group) writes its own partial row; the host sums the (gridDim.x * rpb, cols) partials
    if (threadIdx.x < rpb * W) {
        float* prow = col_sum + ((size_t)blockIdx.x * rpb + r0) * (size_t)(ELEM == 4 ? W : 2 * W);
        if constexpr (ELEM == 4) prow[wc] = s0;
        else { prow[2 * wc] = s0; prow[2 * wc + 1] = s1; }
    }
}

// ---------------------------------------------------------------------------------------- row 8 (Ref-NeRF render path)
// coarseFineMerge's sort (nerf_base.py:59-73) for the render path: the K fine depths come sorted out of the resampling and the C
// coarse ones are stratified, so the sort of their concatenation is normally a MERGE: element i of `a` goes to i + #(b < a_i),
// element j of `b` to j + #(a <= b_j) (binary searches in LDS).  The last merged depth is dropped.  Sorted VALUES are independent of
// how ties are ordered, so z_out equals torch.sort(cat(a, b))[0][:, :-1] bit for bit.  The stratified depths are only ascending
// while the jitter (far - near) / n_fine does not exceed the spacing of the 64 bins, i.e. for n_fine >= 63: a wave that finds one
// of its inputs out of order first sorts it in LDS (stable rank sort, O(n^2 / 64) per lane -- the rare path).
// (idx / itmp, both or neither: a row of source indices that moves with the values -- merge_sorted_order_kernel's)
DEVINL void wave_sort_if_needed(float* v, float* tmp, int n, int lane, int* idx = nullptr, int* itmp = nullptr) {
    int bad = 0;
    for (int i = lane; i + 1 < n; i += 64) bad |= (v[i] > v[i + 1]) ? 1 : 0;
    if (!__any(bad)) return;
    for (int i = lane; i < n; i += 64) {
        const float x = v[i];
        int r = 0;
        for (int k = 0; k < n; ++k) { const float y = v[k]; r += (y < x || (y == x && k < i)) ? 1 : 0; }
        tmp[r] = x;
        if (idx) itmp[r] = idx[i];
    }
    lds_wave_sync();
    for (int i = lane; i < n; i += 64) { v[i] = tmp[i]; if (idx) idx[i] = itmp[i]; }
    lds_wave_sync();
}
// The rank searches of the merge (and of the interlevel loss): binary searches over an ascending row of n floats.
DEVINL int count_le(const float* a, int n, float v) {                                        // #{k < n : a_k <= v}
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
DEVINL int count_lt(const float* a, int n, float v) {                                        // #{k < n : a_k < v}
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <class T> static inline __host__ __device__ T merge_lds_floats(T K, T C, bool order) { return (order ? 4 : 2) * (K + C); }   // per wave: la[K] lb[C] tmp[K + C] (order: + indices)
__global__ __launch_bounds__(256) void merge_sorted_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t N, int K, int C,
                                                           float* __restrict__ out) {
    float* la = reinterpret_cast<float*>(smem) + wave_in_block() * merge_lds_floats(K, C, false);
    float* lb = la + K;
    float* tmp = lb + C;                                        // K + C floats of scratch for the rare sorting path
    const int lane = lane_id();
    const int T = K + C - 1;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        for (int i = lane; i < K; i += 64) la[i] = a[n * K + i];
        for (int j = lane; j < C; j += 64) lb[j] = b[n * C + j];
        lds_wave_sync();
        wave_sort_if_needed(la, tmp, K, lane);
        wave_sort_if_needed(lb, tmp, C, lane);
        float* o = out + n * T;
        for (int i = lane; i < K; i += 64) {
            const float v = la[i];
            const int p = i + count_lt(lb, C, v);               // #(b < v)
            if (p < T) o[p] = v;
        }
        for (int j = lane; j < C; j += 64) {
            const float v = lb[j];
            const int p = j + count_le(la, K, v);               // #(a <= v)
            if (p < T) o[p] = v;
        }
    }
}

// The same merge with its sort order, for the training path (train.py:176: coarseFineMerge(..., below_idxs) -> all_inds for getBounds,
// sort_inds for RefNeRF.coarse_grad_select).  order (N, K + C) = the STABLE argsort of cat(a, b) -- fine index i before coarse index
// K + j among equal depths, which is what the device radix sort behind torch.sort produces --, all_inds = gather(cat(f_inds, 0..C-1), order).
// The two rank searches are count_lt / count_le written out: through the calls this kernel measured 1346.6 us against 1339.2 us per
// 640 000 rays (K = 129, C = 64), outside the spread of 4.7 us, and 0.5 to 0.9 % slower in every run; the sort is the shared one.
__global__ __launch_bounds__(256) void merge_sorted_order_kernel(const float* __restrict__ a, const float* __restrict__ b, const int64_t* __restrict__ f_inds,
                                                                 int64_t N, int K, int C, float* __restrict__ out, int64_t* __restrict__ order,
                                                                 int64_t* __restrict__ all_inds) {
    float* la = reinterpret_cast<float*>(smem) + wave_in_block() * merge_lds_floats(K, C, true);
    float* lb = la + K;
    float* tmp = lb + C;
    int* ia = reinterpret_cast<int*>(tmp + K + C);
    int* ib = ia + K;
    int* itmp = ib + C;
    const int lane = lane_id();
    const int T = K + C - 1;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        for (int i = lane; i < K; i += 64) { la[i] = a[n * K + i]; ia[i] = i; }
        for (int j = lane; j < C; j += 64) { lb[j] = b[n * C + j]; ib[j] = K + j; }
        lds_wave_sync();
        wave_sort_if_needed(la, tmp, K, lane, ia, itmp);
        wave_sort_if_needed(lb, tmp, C, lane, ib, itmp);
        float* o = out + n * T;
        int64_t* ord = order + n * (K + C);
        int64_t* ai = all_inds ? all_inds + n * (K + C) : nullptr;
        for (int i = lane; i < K; i += 64) {
            const float v = la[i];
            int lo = 0, hi = C;                                 // #(b < v)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (lb[mid] < v) lo = mid + 1; else hi = mid; }
            const int p = i + lo, src = ia[i];
            if (p < T) o[p] = v;
            ord[p] = src;
            if (ai) ai[p] = f_inds[n * K + src];
        }
        for (int j = lane; j < C; j += 64) {
            const float v = lb[j];
            int lo = 0, hi = K;                                 // #(a <= v)
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (la[mid] <= v) lo = mid + 1; else hi = mid; }
            const int p = j + lo, src = ib[j];
            if (p < T) o[p] = v;
            ord[p] = src;
            if (ai) ai[p] = src - K;
        }
    }
}

// RefNeRF.coarse_grad_select (ref_model.py:108-117): out[n, k] = grads[n, p_k], p_k the k-th position (ascending) whose sort index is
// flagged (>= T - c_pnum: the reference's mask cat(zeros(T - c), ones(c)) gathered by the sort order); should a row hold fewer than c_pnum
// flagged positions, the unflagged ones follow in order -- exactly what the reference's boolean mask does when the row counts agree and
// what a stable descending sort of the flags does otherwise.  One wavefront per ray, ranks by ballot.
__global__ __launch_bounds__(256) void coarse_grad_select_kernel(const float* __restrict__ grads, const int64_t* __restrict__ sort_inds, int64_t N, int T, int D,
                                                                 int c_pnum, float* __restrict__ out) {
    const int lane = lane_id();
    const int64_t thr = (int64_t)T - c_pnum;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        const int64_t* si = sort_inds + n * T;
        const float* g = grads + n * (int64_t)T * D;
        float* o = out + n * (int64_t)c_pnum * D;
        int base = 0;
        for (int want = 1; want >= 0; --want) {                // flagged positions first, then the others
            for (int p0 = 0; p0 < T && base < c_pnum; p0 += 64) {
                const int p = p0 + lane;
                const bool hit = p < T && ((si[p] >= thr) == (want == 1));
                const unsigned long long m = __ballot(hit);
                const int k = base + __popcll(m & ((1ull << lane) - 1ull));
                if (hit && k < c_pnum)
                    for (int d = 0; d < D; ++d) o[(int64_t)k * D + d] = g[(int64_t)p * D + d];
                base += __popcll(m);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------- Ref-NeRF's normal losses (ref_model.py:127-143)
// WeightedNormalLoss: sum w (1 - <d_norm, p_norm>)  (mode 0);  BackFaceLoss: mean w relu(<normal, ray_d>)  (mode 1; the mean's 1 / M is `scale`).
// One streaming pass + a fixed-order two-stage sum (block partials, then one block) -- deterministic -- instead of the reference's
// five element-wise torch launches per loss; the backward is one pass too (a product rule per element).
constexpr int LOSS_BLOCKS = 256;
// The losses' fixed-order fp64 block sum: every wave's wave_sum_d into `red` (LDS, one slot per wave and value), then THREAD 0 adds the
// slots in wave order, ((0 + 1) + 2) + 3 -- its result is the sum, every other thread's is left as it was.  A caller whose `red` aliases
// rows that are still being read puts a __syncthreads() in front.
DEVINL double block_sum_d(double acc, double* red, int waves = WAVES_PER_BLOCK) {
    acc = wave_sum_d(acc);
    if (lane_id() == 0) red[wave_in_block()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = red[0];
        for (int k = 1; k < waves; ++k) acc += red[k];
    }
    return acc;
}
// the same for two values at once (slots interleaved), four waves
DEVINL void block_sum2_d(double& p, double& q, double* red) {
    p = wave_sum_d(p);
    q = wave_sum_d(q);
    if (lane_id() == 0) { red[2 * wave_in_block()] = p; red[2 * wave_in_block() + 1] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        p = ((red[0] + red[2]) + red[4]) + red[6];
        q = ((red[1] + red[3]) + red[5]) + red[7];
    }
}
DEVINL float dot_loss_term(float x, int mode) { return mode == 0 ? 1.0f - x : (x > 0.0f ? x : 0.0f); }
__global__ __launch_bounds__(256) void weighted_dot_loss_kernel(const float* __restrict__ w, const float* __restrict__ a, const float* __restrict__ b, int64_t M,
                                                                int mode, float* __restrict__ partial) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const float x = (a[3 * i] * b[3 * i] + a[3 * i + 1] * b[3 * i + 1]) + a[3 * i + 2] * b[3 * i + 2];
        acc += (double)(w[i] * dot_loss_term(x, mode));
    }
    acc = block_sum_d(acc, reinterpret_cast<double*>(smem));
    if (threadIdx.x == 0) reinterpret_cast<double*>(partial)[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void weighted_dot_loss_final_kernel(const float* __restrict__ partial, int n, float scale, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += reinterpret_cast<const double*>(partial)[i];
    acc = block_sum_d(acc, reinterpret_cast<double*>(smem));
    if (threadIdx.x == 0) out[0] = (float)(acc * (double)scale);
}
__global__ void weighted_dot_loss_backward_kernel(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ a, const float* __restrict__ b,
                                                  int64_t M, int mode, float scale, float* __restrict__ d_w, float* __restrict__ d_a, float* __restrict__ d_b) {
    const float gs = g[0] * scale;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < M; i += (int64_t)gridDim.x * blockDim.x) {
        const float ax = a[3 * i], ay = a[3 * i + 1], az = a[3 * i + 2], bx = b[3 * i], by = b[3 * i + 1], bz = b[3 * i + 2];
        const float x = (ax * bx + ay * by) + az * bz;
        if (d_w) d_w[i] = gs * dot_loss_term(x, mode);
        const float k = gs * w[i] * (mode == 0 ? -1.0f : (x > 0.0f ? 1.0f : 0.0f));      // d term / d x, times the weight
        if (d_a) { d_a[3 * i] = k * bx; d_a[3 * i + 1] = k * by; d_a[3 * i + 2] = k * bz; }
        if (d_b) { d_b[3 * i] = k * ax; d_b[3 * i + 1] = k * ay; d_b[3 * i + 2] = k * az; }
    }
}

// ---------------------------------------------------------------------------------------- distortion regularisers (include/nerf_amd.h)
// Per ray M = S - 1 intervals with centres c_i, weights a_i and widths d_i = t_i+1 - t_i:
//   mode 0  Regularizer (addtional.py:26-35): c = (t_i + t_i+1) / 2, a = (w_i + w_i+1) / 2, r_i = sqrt(sum_j (c_i - c_j)^2)
//   mode 1  Mip-NeRF 360 L_dist:              c = (e_i + e_i+1) / 2, a = w_i,               r_i = 1
//   P = sum_ij a_i a_j |c_i - c_j| / r_i,  Q = sum_i d_i a_i^2;  the mode's normalisation (dist_coeffs) turns sum P, sum Q into the loss.
// One wavefront per ray: the row's (c, a) pairs staged in LDS in fp32 (any order: nothing assumes sorted depths), each lane owns DIST_R
// intervals and walks every j with broadcast LDS reads, the pair sums in fp64.  The reference's expression materialises (N, M, M) tensors.
// Backward (s_kj = sgn(c_k - c_j), sgn(0) = 0; u = a / r, q = a D / r^3, D_k = sum_j a_j |c_k - c_j|):
//   dP/da_k = D_k / r_k + sum_i u_i |c_i - c_k|,   dP/dc_k = u_k sum_j a_j s_kj + a_k sum_i u_i s_ki - q_k sum_j (c_k - c_j) - sum_i q_i (c_k - c_i)
//   dQ/da_k = 2 d_k a_k,  dQ/dd_k = a_k^2;  then the 2-tap averages / differences scatter to columns k and k + 1 of w and t.
// Mode 0 needs u and q of every interval: a first pass stores them next to (c, a) in fp64 -- the depth gradient's four terms cancel where
// centres come close (exactly with two intervals, where P is constant in t), and fp32 rows of u, q left ~1e-7 / |c_i - c_j| of its largest
// entry --, 24 bytes per interval; mode 1 (r = 1, q = 0) is one pass over fp32 (c, a).
constexpr int DIST_R = 2;
constexpr int DIST_BLOCKS = 1024;                    // forward grid cap: the workspace's (P, Q) partial pairs (NERF_AMD_DISTORTION_WORKSPACE_FLOATS / 4)
DEVINL void dist_coeffs(int mode, int64_t N, int M, double& cP, double& cQ) {
    if (mode == 0) { cP = 1.0 / ((double)N * M * M); cQ = 1.0 / (3.0 * N * M); }     // torch.mean over (N, M, M) and over (N, M), / 3
    else { cP = 1.0 / (double)N; cQ = 1.0 / (3.0 * N); }
}
// row[W i] = c_i, row[W i + 1] = a_i for the M intervals of ray n
template <int MODE, int W>
DEVINL void dist_stage(const float* __restrict__ w, const float* __restrict__ t, int64_t n, int S, float* row) {
    const int M = S - 1;
    const float* tn = t + n * S;
    const float* wn = w + n * (MODE == 0 ? S : M);
    for (int i = lane_id(); i < M; i += 64) {
        row[W * i] = (tn[i] + tn[i + 1]) / 2.0f;
        row[W * i + 1] = MODE == 0 ? (wn[i] + wn[i + 1]) / 2.0f : wn[i];
    }
}

static inline __host__ __device__ size_t dist_wave_floats(int W, int M) { return (size_t)W * M; }   // per wave: W floats for each of the M intervals
template <int MODE>
__global__ __launch_bounds__(256) void distortion_loss_kernel(const float* __restrict__ w, const float* __restrict__ t, int64_t N, int S,
                                                              double* __restrict__ partial) {
    const int M = S - 1, lane = lane_id();
    float* row = reinterpret_cast<float*>(smem) + (size_t)wave_in_block() * 2 * M;   // = wave x dist_wave_floats(2, M), kept spelled out: through the call the compiler schedules this kernel differently
    double accP = 0.0, accQ = 0.0;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        dist_stage<MODE, 2>(w, t, n, S, row);
        lds_wave_sync();
        const float* tn = t + n * S;
        for (int base = 0; base < M; base += 64 * DIST_R) {
            float ci[DIST_R];
            double D[DIST_R], R2[DIST_R];
#pragma unroll
            for (int r = 0; r < DIST_R; ++r) {
                const int i = base + 64 * r + lane;
                ci[r] = row[2 * (i < M ? i : M - 1)];
                D[r] = 0.0; R2[r] = 0.0;
            }
#pragma unroll 4
            for (int j = 0; j < M; ++j) {
                const float2 cj = reinterpret_cast<const float2*>(row)[j];
                const double aj = (double)cj.y;
#pragma unroll
                for (int r = 0; r < DIST_R; ++r) {
                    const float d = ci[r] - cj.x;
                    D[r] = fma(aj, (double)fabsf(d), D[r]);
                    if (MODE == 0) R2[r] = fma((double)d, (double)d, R2[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < DIST_R; ++r) {
                const int i = base + 64 * r + lane;
                if (i < M) {
                    const double a = (double)row[2 * i + 1];
                    accP += MODE == 0 ? a * D[r] / sqrt(R2[r]) : a * D[r];                  // r_i = 0 (coincident centres): 0/0 = NaN, as the reference
                    accQ += (double)(tn[i + 1] - tn[i]) * a * a;
                }
            }
        }
    }
    __syncthreads();                                                                         // (the rows' LDS becomes the block's reduction slots)
    block_sum2_d(accP, accQ, reinterpret_cast<double*>(smem));
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = accP; partial[2 * blockIdx.x + 1] = accQ; }
}
__global__ __launch_bounds__(256) void distortion_loss_final_kernel(const double* __restrict__ partial, int n, int64_t N, int M, int mode, float scale,
                                                                    float* __restrict__ out) {
    double p = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { p += partial[2 * i]; q += partial[2 * i + 1]; }
    block_sum2_d(p, q, reinterpret_cast<double*>(smem));
    if (threadIdx.x == 0) {
        double cP, cQ;
        dist_coeffs(mode, N, M, cP, cQ);
        out[0] = (float)((p * cP + q * cQ) * (double)scale);
    }
}

// dL/d(column k) = the interval-k part h plus the interval-(k-1) part l of the lane below (lane 0: `carry`, lane 63 of the previous register)
DEVINL double dist_from_below(double l, double& carry) {
    double below = __shfl_up(l, 1, 64);
    if (lane_id() == 0) below = carry;
    carry = __shfl(l, 63, 64);
    return below;
}
template <int MODE>
__global__ __launch_bounds__(256) void distortion_loss_backward_kernel(const float* __restrict__ w, const float* __restrict__ t, int64_t N, int S,
                                                                       float scale, const float* __restrict__ g, float* __restrict__ d_w,
                                                                       float* __restrict__ d_t) {
    constexpr int W = MODE == 0 ? 6 : 2;                                                     // LDS floats per interval: c, a (, u, q as doubles)
    const int M = S - 1, lane = lane_id();
    float* row = reinterpret_cast<float*>(smem) + wave_in_block() * dist_wave_floats(W, M);
    double kP, kQ;
    dist_coeffs(MODE, N, M, kP, kQ);
    const double gs = (double)g[0] * (double)scale;
    kP *= gs; kQ *= gs;
    for (int64_t n = blockIdx.x * (int64_t)WAVES_PER_BLOCK + wave_in_block(); n < N; n += (int64_t)gridDim.x * WAVES_PER_BLOCK) {
        lds_wave_sync();
        dist_stage<MODE, W>(w, t, n, S, row);
        lds_wave_sync();
        const float* tn = t + n * S;
        if (MODE == 0) {                                                                     // pass 1: u_i = a_i / r_i, q_i = a_i D_i / r_i^3 into the row
            for (int base = 0; base < M; base += 64 * DIST_R) {
                float ci[DIST_R];
                double D[DIST_R], R2[DIST_R];
#pragma unroll
                for (int r = 0; r < DIST_R; ++r) {
                    const int i = base + 64 * r + lane;
                    ci[r] = row[W * (i < M ? i : M - 1)];
                    D[r] = 0.0; R2[r] = 0.0;
                }
#pragma unroll 4
                for (int j = 0; j < M; ++j) {
                    const float2 cj = *reinterpret_cast<const float2*>(row + W * j);
                    const double aj = (double)cj.y;
#pragma unroll
                    for (int r = 0; r < DIST_R; ++r) {
                        const float d = ci[r] - cj.x;
                        D[r] = fma(aj, (double)fabsf(d), D[r]);
                        R2[r] = fma((double)d, (double)d, R2[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < DIST_R; ++r) {
                    const int i = base + 64 * r + lane;
                    if (i < M) {
                        const double a = (double)row[W * i + 1], rr = sqrt(R2[r]);
                        double* uq = reinterpret_cast<double*>(row + W * i + 2);
                        uq[0] = a / rr;
                        uq[1] = a * D[r] / (rr * R2[r]);
                    }
                }
            }
            lds_wave_sync();
        }
        double carry_w = 0.0, carry_t = 0.0;
        for (int base = 0; base < M; base += 64 * DIST_R) {
            float ck[DIST_R];
            double D[DIST_R], R2[DIST_R], E[DIST_R], Sg[DIST_R], T[DIST_R], V[DIST_R], Cs[DIST_R];
#pragma unroll
            for (int r = 0; r < DIST_R; ++r) {
                const int k = base + 64 * r + lane;
                ck[r] = row[W * (k < M ? k : M - 1)];
                D[r] = R2[r] = E[r] = Sg[r] = T[r] = V[r] = Cs[r] = 0.0;
            }
            if (MODE == 0) {
#pragma unroll 2
                for (int j = 0; j < M; ++j) {
                    const float2 x = *reinterpret_cast<const float2*>(row + W * j);          // (c_j, a_j), then (u_j, q_j) in fp64
                    const double* uq = reinterpret_cast<const double*>(row + W * j + 2);      // (8-byte aligned: 24-byte intervals)
                    const double aj = (double)x.y, uj = uq[0], qj = uq[1];
#pragma unroll
                    for (int r = 0; r < DIST_R; ++r) {
                        const float d = ck[r] - x.x;
                        const double ad = (double)fabsf(d), dd = (double)d, s = (double)((d > 0.0f) - (d < 0.0f));
                        D[r] = fma(aj, ad, D[r]);
                        R2[r] = fma(dd, dd, R2[r]);
                        E[r] = fma(uj, ad, E[r]);
                        Sg[r] = fma(aj, s, Sg[r]);
                        T[r] = fma(uj, s, T[r]);
                        V[r] = fma(qj, dd, V[r]);
                        Cs[r] += dd;
                    }
                }
            } else {
#pragma unroll 4
                for (int j = 0; j < M; ++j) {
                    const float2 x = *reinterpret_cast<const float2*>(row + W * j);
                    const double aj = (double)x.y;
#pragma unroll
                    for (int r = 0; r < DIST_R; ++r) {
                        const float d = ck[r] - x.x;
                        D[r] = fma(aj, (double)fabsf(d), D[r]);
                        Sg[r] += (double)(d > 0.0f ? x.y : (d < 0.0f ? -x.y : 0.0f));
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < DIST_R; ++r) {
                const int k = base + 64 * r + lane;
                double ga = 0.0, gc = 0.0, gd = 0.0;
                if (k < M) {
                    const double a = (double)row[W * k + 1], dk = (double)(tn[k + 1] - tn[k]);
                    if (MODE == 0) {
                        const double rr = sqrt(R2[r]), u = a / rr, q = a * D[r] / (rr * R2[r]);
                        ga = kP * (D[r] / rr + E[r]);
                        gc = kP * (((u * Sg[r] + a * T[r]) - q * Cs[r]) - V[r]);
                    } else {
                        ga = kP * (2.0 * D[r]);
                        gc = kP * (2.0 * a * Sg[r]);
                    }
                    ga += kQ * (2.0 * dk * a);
                    gd = kQ * (a * a);
                }
                // column k of t: 0.5 gc_k - gd_k + (0.5 gc_k-1 + gd_k-1);  mode 0, column k of w: 0.5 ga_k + 0.5 ga_k-1
                const double lt = 0.5 * gc + gd, lw = 0.5 * ga;
                const double bt = dist_from_below(lt, carry_t), bw = dist_from_below(lw, carry_w);
                if (k <= M) {                                                                // (k = M: the last column, its interval part is 0)
                    if (d_t) d_t[n * S + k] = (float)((0.5 * gc - gd) + bt);
                    if (MODE == 0 && d_w) d_w[n * S + k] = (float)(lw + bw);
                }
                if (MODE == 1 && d_w && k < M) d_w[n * M + k] = (float)ga;
            }
        }
        if (M % (64 * DIST_R) == 0 && lane == 0) {                                           // column M fell past the last register block
            if (d_t) d_t[n * S + M] = (float)carry_t;
            if (MODE == 0 && d_w) d_w[n * S + M] = (float)carry_w;
        }
    }
}

// ---------------------------------------------------------------------------------------- interlevel loss L_prop (include/nerf_amd.h)
// One wavefront per ray.  Per wave in LDS: c[K+1] (fp64 exclusive prefix sum of w_prop), F[M+1] (backward only: fp64 prefix sum of the
// per-interval factors), tf[M+1] (fine edges), te[K+1] (proposal edges, +inf appended in the open form): 12 (M + K + 2) bytes at most,
// 24.6 KB at M = K = 1024.  Up to IL_WAVE_BUDGET per wave the workgroup holds four waves (64 KiB of LDS), above it two (il_waves).
// Every search is a binary search over an ascending LDS row whose result is clamped into the row, so rows that are not ascending
// (or NaN) give some bound, never an access outside the row.
constexpr int IL_BLOCKS = 1024;                      // forward grid cap: the workspace's fp64 partials (NERF_AMD_INTERLEVEL_WORKSPACE_FLOATS / 2)
constexpr size_t IL_WAVE_BUDGET = 16 * 1024;
static inline __host__ __device__ size_t il_wave_bytes(int M, int K, bool bwd) {
    const size_t b = (size_t)8 * (K + 1) + (bwd ? (size_t)8 * (M + 1) : 0) + (size_t)4 * (M + K + 2);
    return (b + 7) & ~(size_t)7;
}
static inline int il_waves(int M, int K, bool bwd) { return il_wave_bytes(M, K, bwd) <= IL_WAVE_BUDGET ? 4 : 2; }
struct IlRows { double* c; double* F; float* tf; float* te; };
DEVINL IlRows il_rows(int M, int K, bool bwd) {
    IlRows r;
    r.c = reinterpret_cast<double*>(smem + (size_t)wave_in_block() * il_wave_bytes(M, K, bwd));
    r.F = r.c + (K + 1);
    r.tf = reinterpret_cast<float*>(r.F + (bwd ? M + 1 : 0));
    r.te = r.tf + (M + 1);
    return r;
}
// the wave's rows of ray n: edges as they are, c by a wave scan per 64 columns with the running total carried over (a fixed order)
DEVINL void il_stage(const float* __restrict__ t, const float* __restrict__ w_prop, const float* __restrict__ t_prop, int64_t n, int M, int K, int Kp,
                     const IlRows& r) {
    const int lane = lane_id();
    const float* tn = t + n * (M + 1);
    const float* en = t_prop + n * Kp;
    const float* pn = w_prop + n * K;
    for (int i = lane; i <= M; i += 64) r.tf[i] = tn[i];
    for (int j = lane; j <= K; j += 64) r.te[j] = j < Kp ? en[j] : __builtin_inff();
    if (lane == 0) r.c[0] = 0.0;
    double carry = 0.0;
    for (int base = 0; base < K; base += 64) {
        const int j = base + lane;
        const double v = wave_incl_scan_add(j < K ? (double)pn[j] : 0.0) + carry;
        if (j < K) r.c[j + 1] = v;
        carry = wave_last(v);
    }
}
DEVINL double il_bound(const IlRows& r, int K, int i) {
    const int cl = count_le(r.te, K + 1, r.tf[i]), ch = count_le(r.te, K + 1, r.tf[i + 1]);
    return r.c[ch < K ? ch : K] - r.c[cl > 0 ? cl - 1 : 0];                                  // c[hi(t_i+1)] - c[lo(t_i)]
}

__global__ __launch_bounds__(256) void interlevel_loss_kernel(const float* __restrict__ w, const float* __restrict__ t, const float* __restrict__ w_prop,
                                                              const float* __restrict__ t_prop, int64_t N, int M, int K, int Kp,
                                                              double* __restrict__ partial, float* __restrict__ bounds_out) {
    const int waves = (int)(blockDim.x >> 6), lane = lane_id();
    const IlRows r = il_rows(M, K, false);
    double acc = 0.0;
    for (int64_t n = blockIdx.x * (int64_t)waves + wave_in_block(); n < N; n += (int64_t)gridDim.x * waves) {
        lds_wave_sync();
        il_stage(t, w_prop, t_prop, n, M, K, Kp, r);
        lds_wave_sync();
        const float* wn = w + n * M;
        for (int i = lane; i < M; i += 64) {
            const double b = il_bound(r, K, i), wi = (double)wn[i];
            const double d = wi - b > 0.0 ? wi - b : 0.0;
            acc += d * d / (wi + 1e-8);
            if (bounds_out) bounds_out[n * M + i] = (float)b;
        }
    }
    __syncthreads();                                                                         // (the rows' LDS becomes the block's reduction slots)
    acc = block_sum_d(acc, reinterpret_cast<double*>(smem), waves);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void interlevel_loss_final_kernel(const double* __restrict__ partial, int n, float scale, float* __restrict__ out) {
    double p = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) p += partial[i];
    p = block_sum_d(p, reinterpret_cast<double*>(smem));
    if (threadIdx.x == 0) out[0] = (float)(p * (double)scale);
}
__global__ __launch_bounds__(256) void interlevel_loss_backward_kernel(const float* __restrict__ w, const float* __restrict__ t,
                                                                       const float* __restrict__ w_prop, const float* __restrict__ t_prop, int64_t N,
                                                                       int M, int K, int Kp, float scale, const float* __restrict__ g,
                                                                       float* __restrict__ d_w_prop) {
    const int waves = (int)(blockDim.x >> 6), lane = lane_id();
    const IlRows r = il_rows(M, K, true);
    const double gs = (double)g[0] * (double)scale;
    for (int64_t n = blockIdx.x * (int64_t)waves + wave_in_block(); n < N; n += (int64_t)gridDim.x * waves) {
        lds_wave_sync();
        il_stage(t, w_prop, t_prop, n, M, K, Kp, r);
        lds_wave_sync();
        const float* wn = w + n * M;
        if (lane == 0) r.F[0] = 0.0;                                                         // F_i = sum_{i' < i} -2 relu(w_i' - bound_i') / (w_i' + 1e-8)
        double carry = 0.0;
        for (int base = 0; base < M; base += 64) {
            const int i = base + lane;
            double f = 0.0;
            if (i < M) {
                const double wi = (double)wn[i], d = wi - il_bound(r, K, i);
                if (d > 0.0) f = -2.0 * d / (wi + 1e-8);
            }
            f = wave_incl_scan_add(f) + carry;
            if (i < M) r.F[i + 1] = f;
            carry = wave_last(f);
        }
        lds_wave_sync();
        for (int j = lane; j < K; j += 64) {                                                 // the fine intervals over proposal interval j: [i0, i1)
            const int i1 = count_lt(r.tf, M, r.te[j + 1]);                                   //   t_i < e_j+1
            const int i0 = count_lt(r.tf + 1, M, r.te[j]);                                   //   t_i+1 >= e_j
            d_w_prop[n * K + j] = (float)(i1 > i0 ? gs * (r.F[i1] - r.F[i0]) : 0.0);
        }
    }
}

int blocks_for(int64_t work, int per_block) {
    int64_t b = (work + per_block - 1) / per_block;
    const int64_t cap = 256 * 8;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host launchers
// dynamic LDS of the launch a shape leads to = the kernel's own per-wave layout x the waves of a workgroup, in size_t: no shape overflows (capi.hip checks against these)
static size_t wave_rows_bytes(size_t floats_per_wave) { return WAVES_PER_BLOCK * floats_per_wave * 4; }
size_t nk::sk_inverse_sample_lds_bytes(int C, int K) { return wave_rows_bytes(inv_lds_floats(C, K)); }
size_t nk::sk_resample_lds_bytes(int C, int K) { return wave_rows_bytes(rs_lds_floats(C, K)); }
size_t nk::sk_warped_resample_lds_bytes(int C, int K) { return wave_rows_bytes(warped_lds_floats(C, K)); }
size_t nk::sk_resample_window_lds_bytes(int C, int K, int warped) { return wave_rows_bytes(rsw_lds_floats(C, K, warped != 0)); }
size_t nk::sk_get_bounds_lds_bytes(int C) { return wave_rows_bytes(gb_lds_floats((size_t)C)); }
size_t nk::sk_get_bounds_backward_lds_bytes(int K) { return wave_rows_bytes(gbb_lds_words((size_t)K)); }
size_t nk::sk_merge_sorted_lds_bytes(int K, int C, int order) { return wave_rows_bytes(merge_lds_floats((size_t)K, (size_t)C, order != 0)); }
int nk::sk_positional_encoding(const float* x, int64_t M, int L, float* out, hipStream_t st) {
    if (M * L == 0) return 0;
    hipLaunchKernelGGL(pe_kernel, dim3(blocks_for(M, ENC_TILE)), dim3(256), enc_lds_bytes(L), st, x, M, L, out);
    return (int)hipGetLastError();
}
int nk::sk_ipe_feature(const float* z, const float* rays, int64_t N, int Sn, int L, float r2, const float* dir_norm, float* feat, float* mu,
                   float* mu_t, int contract, hipStream_t st) {
    if (N * Sn == 0) return 0;
    hipLaunchKernelGGL(ipe_feature_kernel, dim3(blocks_for(N * Sn, ENC_TILE)), dim3(256), enc_lds_bytes(L), st, z, rays, N, Sn, L, r2, dir_norm, feat, mu, mu_t, contract);
    return (int)hipGetLastError();
}
int nk::sk_cone_parameters(const float* z, int64_t N, int Sn, float r2, float* mu_t, float* var_t, float* var_r, hipStream_t st) {
    if (N * Sn == 0) return 0;
    hipLaunchKernelGGL(cone_parameters_kernel, dim3(blocks_for(N * Sn, 256)), dim3(256), 0, st, z, N, Sn, r2, mu_t, var_t, var_r);
    return (int)hipGetLastError();
}
int nk::sk_dirs_norm(const float* rays, int64_t N, float* out, hipStream_t st) {
    hipLaunchKernelGGL(dirs_norm_kernel, dim3(1), dim3(1024), 0, st, rays, N, out);
    return (int)hipGetLastError();
}
// `partials`: DN_BLOCKS doubles of device scratch (8-byte aligned)
int nk::sk_dirs_norm_scratch(const float* rays, int64_t N, float* out, void* partials, hipStream_t st) {
    hipLaunchKernelGGL(dirs_norm_partial_kernel, dim3(DN_BLOCKS), dim3(256), 0, st, rays, N, reinterpret_cast<double*>(partials));
    hipLaunchKernelGGL(dirs_norm_final_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const double*>(partials), out);
    return (int)hipGetLastError();
}
int nk::sk_train_sampler(const float* rgbs, const int64_t* coords, int64_t P, const float* pose, const float* pose_dev, float fx, float fy, float near, float far,
                     int64_t N, int C, uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, hipStream_t st) {
    if (N == 0) return 0;
    Cam c; c.H = 0; c.W = 0; c.fx = fx; c.fy = fy;
    for (int i = 0; i < 12; ++i) c.pose[i] = pose ? pose[i] : 0.0f;
    hipLaunchKernelGGL(train_sampler_kernel, dim3(blocks_for(N, 4)), dim3(256), 0, st, rgbs, coords, P, c, near, C > 0 ? (far - near) / (float)C : 0.0f, N, C, seed,
                       pts, lengths, rgb, rays, pose_dev, seed_dev);
    return (int)hipGetLastError();
}

// window: x0 <= col < x1, y0 <= row < y1 (validated by the caller)
int nk::sk_scene_sampler(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1, int y0, int y1,
                     float fx, float fy, float near, float far, int64_t N, int C, uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths,
                     float* rgb, float* rays, int64_t* index, hipStream_t st) {
    if (N == 0) return 0;
    const int ww = x1 - x0;
    const int64_t wp = (int64_t)(y1 - y0) * ww;
    hipLaunchKernelGGL(scene_sampler_kernel, dim3(blocks_for(N, 4)), dim3(256), 0, st, images, poses, V, H, W, view_ids, K, x0, ww, y0, wp, fx, fy, near,
                       C > 0 ? (far - near) / (float)C : 0.0f, N, C, seed, seed_dev, pts, C > 0 ? lengths : nullptr, rgb, rays, index);
    return (int)hipGetLastError();
}

// `cameras`: (V, NERF_AMD_CAMERA_ROW) on the device; the window as in sk_scene_sampler
int nk::sk_scene_sampler_camera(const float* images, const float* poses, const float* cameras, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0,
                            int x1, int y0, int y1, float near, float far, int64_t N, int C, uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths,
                            float* rgb, float* rays, int64_t* index, hipStream_t st) {
    if (N == 0) return 0;
    const int ww = x1 - x0;
    const int64_t wp = (int64_t)(y1 - y0) * ww;
    hipLaunchKernelGGL(scene_sampler_camera_kernel, dim3(blocks_for(N, 4)), dim3(256), 0, st, images, poses, cameras, V, H, W, view_ids, K, x0, ww, y0, wp, near,
                       C > 0 ? (far - near) / (float)C : 0.0f, N, C, seed, seed_dev, pts, C > 0 ? lengths : nullptr, rgb, rays, index);
    return (int)hipGetLastError();
}

// Philox uniforms as a tensor, u (N,K) = the inverse-CDF stream of device_common.h (philox_u_inv) -- for callers that keep the
// reference's op-by-op structure (inverseSample(weights, depths, u)) but want the draw on the device and, with `seed_dev`, replayable
// from a captured graph.  One thread per element.
// (ABI 121) `ray_offset`: row n of the tensor is GLOBAL ray ray_offset + n (a chunk / shard of a larger ray list draws the bits the whole
// list would); `strat`: the stratified-jitter stream u_strat(n, s) (word 0 of the ray's blocks) instead of the inverse-CDF stream
__global__ void philox_uniforms_kernel(float* __restrict__ out, int64_t N, int K, uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                       int64_t ray_offset, int strat) {
    if (seed_dev != nullptr) seed = seed_dev[0];
    const int64_t total = N * K;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / K;
        const int k = (int)(i - n * K);
        out[i] = strat ? philox_u_strat(seed, ray_offset + n, k) : philox_u_inv(seed, ray_offset + n, k);
    }
}
// The bottle-neck perturbation of Ref-NeRF's training forward as a tensor, out (M, 128) ~ N(0, std): bit-identical to what ref_kernel
// draws in place for the same key and sample index (device_common.h philox_normal8) -- for tests, the layer-by-layer route and callers
// that want the reference's explicit `spa_info_b + noise` (ref_model.py:84-85).  One thread per (sample, block of eight deviates).
__global__ void philox_normal_kernel(float* __restrict__ out, int64_t M, uint64_t seed, const uint64_t* __restrict__ seed_dev, float std, int64_t sample_offset) {
    if (seed_dev != nullptr) seed = seed_dev[0];
    const int64_t total = M * 16;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i >> 4;
        const int q = (int)(i & 15);
        float z[8];
        philox_normal8(seed, sample_offset + m, q, std, z);
        float* row = out + m * 128 + 16 * (q >> 1) + 4 * (q & 1);
        *reinterpret_cast<f32x4*>(row) = f32x4{z[0], z[1], z[2], z[3]};
        *reinterpret_cast<f32x4*>(row + 8) = f32x4{z[4], z[5], z[6], z[7]};
    }
}
int nk::sk_philox_normal(float* out, int64_t M, uint64_t seed, const uint64_t* seed_dev, float std, int64_t sample_offset, hipStream_t st) {
    if (M == 0) return 0;
    hipLaunchKernelGGL(philox_normal_kernel, dim3(blocks_for(M * 16, 256)), dim3(256), 0, st, out, M, seed, seed_dev, std, sample_offset);
    return (int)hipGetLastError();
}
// seed <- a new, unrelated key for the next step (golden-ratio increment + a xorshift-multiply mix); one thread
__global__ void advance_seed_kernel(uint64_t* __restrict__ seed_dev) {
    uint64_t x = seed_dev[0] + 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    seed_dev[0] = x ^ (x >> 31);
}
int nk::sk_philox_uniforms(float* out, int64_t N, int K, uint64_t seed, const uint64_t* seed_dev, int64_t ray_offset, int strat, hipStream_t st) {
    if (N * K == 0) return 0;
    hipLaunchKernelGGL(philox_uniforms_kernel, dim3(blocks_for(N * K, 256)), dim3(256), 0, st, out, N, K, seed, seed_dev, ray_offset, strat);
    return (int)hipGetLastError();
}
int nk::sk_advance_seed(uint64_t* seed_dev, hipStream_t st) {
    hipLaunchKernelGGL(advance_seed_kernel, dim3(1), dim3(1), 0, st, seed_dev);
    return (int)hipGetLastError();
}
int nk::sk_generate_rays(const float* pose, int H, int W, float fx, float fy, int64_t first, int64_t count, float* rays,
                     hipStream_t st) {
    Cam c; c.H = H; c.W = W; c.fx = fx; c.fy = fy;
    for (int i = 0; i < 12; ++i) c.pose[i] = pose[i];
    if (count == 0) return 0;
    hipLaunchKernelGGL(raygen_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, c, first, count, rays);
    return (int)hipGetLastError();
}
// `camera`: a HOST row of NERF_AMD_CAMERA_ROW floats (validated by the caller)
int nk::sk_generate_rays_camera(const float* pose, int H, int W, const float* camera, int64_t first, int64_t count, float* rays, hipStream_t st) {
    Cam c; c.H = H; c.W = W; c.fx = camera[0]; c.fy = camera[1];
    for (int i = 0; i < 12; ++i) c.pose[i] = pose[i];
    CameraRow row;
    for (int i = 0; i < NERF_AMD_CAMERA_ROW; ++i) row.v[i] = camera[i];
    if (count == 0) return 0;
    hipLaunchKernelGGL(raygen_camera_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, st, row, c, first, count, rays);
    return (int)hipGetLastError();
}
int nk::sk_pixel_rays(const float* pose, float fx, float fy, const int64_t* coords, int64_t N, float* rays, hipStream_t st) {
    Cam c; c.H = 0; c.W = 0; c.fx = fx; c.fy = fy;
    for (int i = 0; i < 12; ++i) c.pose[i] = pose[i];
    if (N == 0) return 0;
    hipLaunchKernelGGL(pixel_rays_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, st, c, coords, N, rays);
    return (int)hipGetLastError();
}
int nk::sk_stratified_points(const float* rays, const float* z_base, const float* u, float jitter, int64_t N, int S, float* z_out,
                         float* pts, hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(stratified_points_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, st, rays, z_base, u, jitter, N, S, z_out, pts);
    return (int)hipGetLastError();
}
int nk::sk_length2pts(const float* rays, const float* z, int64_t N, int S, float* out, hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(length2pts_kernel, dim3(blocks_for(N * S * 6, 256)), dim3(256), 0, st, rays, z, N, S, out);
    return (int)hipGetLastError();
}
int nk::sk_sigma_to_weights(const float* sigma, const float* z, const float* dirs, int64_t N, int S, int act, float* w, hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(sigma_to_weights_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, sigma, z, dirs, N, S, act, w);
    return (int)hipGetLastError();
}
int nk::sk_max_blur(const float* w, int64_t N, int S, float alpha, float* out, hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(max_blur_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, st, w, N, S, alpha, out);
    return (int)hipGetLastError();
}
int nk::sk_inverse_sample(const float* w, const float* z, const float* u, int64_t N, int C, int K, int sort, int mode, float* z_out,
                      int64_t* below, int64_t* above, hipStream_t st) {
    if (N == 0) return 0;
    hipLaunchKernelGGL(inverse_sample_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_inverse_sample_lds_bytes(C, K), st, w, z, u, N, C, K, sort, mode,
                       z_out, below, above);
    return (int)hipGetLastError();
}
int nk::sk_resample(const float* density, const float* z, const float* z_base, const float* u_strat, float z_jitter,
                const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K, int softplus, float alpha,
                uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, int64_t* below, float* w_prop, float* z_coarse, hipStream_t st) {
    if (N == 0) return 0;
    ResampleArgs a{density, z, z_base, u_strat, z_jitter, dirs, dirs_stride, u_inv, N, C, K, softplus, alpha, z_fine, below, w_prop, z_coarse,
                   rng_seed, rng_ray_offset};
    // persistent over rays: exactly one resident round (RS_BLOCKS_PER_CU workgroups fit a CU by registers and LDS at the render shapes),
    // so that no partially filled last round trails behind
    int64_t blocks = (N + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const int64_t resident = (int64_t)nerf_host::cu_count() * RS_BLOCKS_PER_CU;
    if (blocks > resident) blocks = resident;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(256), sk_resample_lds_bytes(C, K), st, a);
    return (int)hipGetLastError();
}
// ---- disparity ray spacing (near, far, gn = fp32(1/near), gf = fp32(1/far): validated and rounded by the caller) ----
int nk::sk_warp_depths(const float* in, const float* rays, int64_t N, int S, int inverse, float near, float far, float gn, float gf, float* out, float* pts,
                   hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(warp_depths_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, st, in, rays, N, S, inverse, WarpConsts{near, far, gn, gf}, out, pts);
    return (int)hipGetLastError();
}
int nk::sk_warped_stratified(const float* rays, const float* u, int64_t N, int C, uint64_t seed, int64_t ray_offset, float near, float far, float gn, float gf,
                         float* s_out, float* z_out, float* pts, hipStream_t st) {
    if (N * C == 0) return 0;
    hipLaunchKernelGGL(warped_stratified_kernel, dim3(blocks_for(N * C, 256)), dim3(256), 0, st, rays, u, N, C, 1.0f / (float)C, seed, ray_offset,
                       WarpConsts{near, far, gn, gf}, s_out, z_out, pts);
    return (int)hipGetLastError();
}
int nk::sk_warped_resample(const float* density, const float* s_c, const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K, int softplus,
                       float alpha, float near, float far, float gn, float gf, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, float* s_fine,
                       int64_t* below, float* w_prop, hipStream_t st) {
    if (N == 0) return 0;
    WarpedResampleArgs a{density, s_c, dirs, dirs_stride, u_inv, N, C, K, softplus, alpha, WarpConsts{near, far, gn, gf}, z_fine, s_fine, below, w_prop,
                         rng_seed, rng_ray_offset};
    hipLaunchKernelGGL(warped_resample_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_warped_resample_lds_bytes(C, K), st, a);
    return (int)hipGetLastError();
}
// ---- the second proposal round: explicit depths, in-kernel uniforms of columns u_col0 .. u_col0 + K - 1 of the inverse-CDF stream ----
int nk::sk_resample_window(const float* density, const float* z, const float* dirs, int dirs_stride, int64_t N, int C, int K, int u_col0, float alpha,
                       uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, hipStream_t st) {
    if (N == 0) return 0;
    ResampleWindowArgs a{density, z, dirs, dirs_stride, N, C, K, u_col0, alpha, WarpConsts{}, z_fine, nullptr, rng_seed, rng_ray_offset};
    hipLaunchKernelGGL(resample_window_kernel<false>, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_resample_window_lds_bytes(C, K, 0), st, a);
    return (int)hipGetLastError();
}
int nk::sk_warped_resample_window(const float* density, const float* s_c, const float* dirs, int dirs_stride, int64_t N, int C, int K, int u_col0, float alpha,
                              float near, float far, float gn, float gf, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, float* s_fine, hipStream_t st) {
    if (N == 0) return 0;
    ResampleWindowArgs a{density, s_c, dirs, dirs_stride, N, C, K, u_col0, alpha, WarpConsts{near, far, gn, gf}, z_fine, s_fine, rng_seed, rng_ray_offset};
    hipLaunchKernelGGL(resample_window_kernel<true>, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_resample_window_lds_bytes(C, K, 1), st, a);
    return (int)hipGetLastError();
}
int nk::sk_composite(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S, int flags,
                 int act, float sigma_shift, float near, float far, const float* normal, const float* cam_dir, float* rgb, float* weights,
                 float* depth, float* normal_img, hipStream_t st) {
    if (N == 0) return 0;
    CompositeArgs a{rgbo, z, z_stride, dirs, dirs_stride, N, S, flags, act, sigma_shift, near, far, normal, cam_dir, rgb, weights, depth, normal_img};
    hipLaunchKernelGGL(composite_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
int nk::sk_composite_rows(const float* rgbo, const int32_t* row_of_ray, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S, int flags,
                      int act, float sigma_shift, float near, float far, const float* normal, const float* cam_dir, float* rgb, float* weights, float* depth,
                      float* normal_img, hipStream_t st) {
    if (N == 0) return 0;
    CompositeArgs a{rgbo, z, z_stride, dirs, dirs_stride, N, S, flags, act, sigma_shift, near, far, normal, cam_dir, rgb, weights, depth, normal_img};
    hipLaunchKernelGGL(composite_rows_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a, row_of_ray);
    return (int)hipGetLastError();
}
// ---- the empty-ray skip: flags -> ordered compaction (three launches behind the flags) / the gather of the alive rays' rows ----
size_t nk::sk_ray_alive_workspace_bytes(int64_t N) {                 // flags (N bytes) | tile counts (ceil(N / 256) ints), each rounded up to 256 bytes, + alignment slack
    const size_t n = (size_t)N, tiles = (n + ALIVE_TILE - 1) / ALIVE_TILE;
    return ((n + 255) & ~(size_t)255) + ((tiles * 4 + 255) & ~(size_t)255) + 256;
}
int nk::sk_ray_alive(const float* density, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int C, double d_min, int32_t* row_of_ray,
                 int64_t* ray_of_row, int64_t* count_dev, void* workspace, hipStream_t st) {
    if (N == 0) return (int)hipMemsetAsync(count_dev, 0, 8, st);
    uint8_t* flags = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) & ~(uintptr_t)255);
    int* tiles = reinterpret_cast<int*>(flags + (((size_t)N + 255) & ~(size_t)255));
    const int64_t n_tiles = (N + ALIVE_TILE - 1) / ALIVE_TILE;
    RayAliveArgs a{density, z, z_stride, dirs, dirs_stride, N, C, d_min, flags};
    hipLaunchKernelGGL(ray_alive_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(alive_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, flags, N, tiles);
    hipLaunchKernelGGL(alive_offsets_kernel, dim3(1), dim3(256), 0, st, tiles, n_tiles, count_dev);
    hipLaunchKernelGGL(alive_tables_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, flags, N, tiles, row_of_ray, ray_of_row);
    return (int)hipGetLastError();
}
int nk::sk_gather_rows(const float* src, int64_t src_stride, const int64_t* ray_of_row, int64_t n_rows, int cols, float* dst, hipStream_t st) {
    if (n_rows * cols == 0) return 0;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks_for(n_rows * cols, 256)), dim3(256), 0, st, src, src_stride, ray_of_row, n_rows, cols, dst);
    return (int)hipGetLastError();
}
int nk::sk_ray_depth_stats(const float* w, const float* z, int z_stride, int closed, const float* dirs, int dirs_stride, int64_t N, int S, int mul_norm,
                           const float* quantiles, int n_quantiles, float near, float far, float* opacity, float* depth_q, hipStream_t st) {
    if (N == 0 || (!opacity && !(depth_q && n_quantiles))) return 0;
    DepthStatsArgs a{w, z, z_stride, closed ? 1 : 0, dirs, dirs_stride, N, S, mul_norm ? 1 : 0, {}, depth_q ? n_quantiles : 0, near, far, opacity, depth_q};
    for (int j = 0; j < a.nq; ++j) a.q[j] = quantiles[j];
    hipLaunchKernelGGL(ray_depth_stats_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
int nk::sk_get_bounds(const float* w, const int64_t* below, int64_t N, int C, int K, float* bounds, hipStream_t st) {
    if (N == 0 || K < 2) return 0;
    hipLaunchKernelGGL(get_bounds_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_get_bounds_lds_bytes(C), st, w, below, N, C, K, bounds);
    return (int)hipGetLastError();
}

// ---- backward launchers ----
int nk::sk_weights_backward(const float* sigma, int sigma_stride, int sigma_off, const float* z, int z_stride, const float* dirs, int dirs_stride,
                        int64_t N, int S, int mul_norm, int act, float sigma_shift, const float* rgbo, const float* d_rgb,
                        const float* d_weights, const float* d_depth, int white_bkg, float near, float far, float* d_sigma,
                        int d_sigma_stride, int d_sigma_off, float* d_rgbo, hipStream_t st) {
    if (N * S == 0) return 0;
    if (S > BWD_MAX_CHUNKS * 64) return (int)hipErrorInvalidValue;
    WeightsBwdArgs a{sigma, sigma_stride, sigma_off, z, z_stride, dirs, dirs_stride, N, S, mul_norm, act, sigma_shift, rgbo, d_rgb, d_weights,
                     d_depth, white_bkg, near, far, d_sigma, d_sigma_stride, d_sigma_off, d_rgbo};
    if (S <= 256) hipLaunchKernelGGL(weights_backward_kernel<4>, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    else if (S <= 512) hipLaunchKernelGGL(weights_backward_kernel<8>, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(weights_backward_kernel<16>, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}
int nk::sk_max_blur_backward(const float* w, const float* g, int64_t N, int S, float* dw, hipStream_t st) {
    if (N * S == 0) return 0;
    hipLaunchKernelGGL(max_blur_backward_kernel, dim3(blocks_for(N * S, 256)), dim3(256), 0, st, w, g, N, S, dw);
    return (int)hipGetLastError();
}
int nk::sk_get_bounds_backward(const int64_t* below, const float* g, int64_t N, int C, int K, float* dw, hipStream_t st) {
    if (N == 0) return 0;
    if (K < 2) { return (int)hipMemsetAsync(dw, 0, (size_t)N * C * 4, st); }
    hipLaunchKernelGGL(get_bounds_backward_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_get_bounds_backward_lds_bytes(K), st, below, g, N, C, K, dw);
    return (int)hipGetLastError();
}
int nk::sk_frag_to_rows(const void* frag, int elem_bytes, int64_t n_sub, int n_kg, int64_t M, void* out, hipStream_t st) {
    if (n_sub == 0 || M == 0) return 0;
    const size_t lds = WAVES_PER_BLOCK * frag_wave_bytes(n_kg, elem_bytes);
    const auto kernel = elem_bytes == 2 ? frag_to_rows_kernel<2> : frag_to_rows_kernel<4>;      // (the opt-in below: the fp32 kernel's alone)
    if (int e = elem_bytes == 2 ? 0 : nerf_host::allow_dynamic_lds(reinterpret_cast<const void*>(kernel), 140 * 1024)) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n_sub, WAVES_PER_BLOCK)), dim3(256), lds, st, (const char*)frag, n_sub, n_kg, M, (char*)out, n_kg * 16);
    return (int)hipGetLastError();
}
int nk::sk_relu_mask(void* delta, const void* act, int elem_bytes, int64_t n, hipStream_t st) {
    if (n == 0) return 0;
    const int64_t words = elem_bytes == 2 ? n / 2 : n;
    if (elem_bytes == 2) hipLaunchKernelGGL(relu_mask_kernel<2>, dim3(blocks_for(words, 256)), dim3(256), 0, st, (uint32_t*)delta, (const uint32_t*)act, words);
    else hipLaunchKernelGGL(relu_mask_kernel<4>, dim3(blocks_for(words, 256)), dim3(256), 0, st, (uint32_t*)delta, (const uint32_t*)act, words);
    return (int)hipGetLastError();
}
int nk::sk_relu_mask_bias(void* delta, const void* act, int elem_bytes, int64_t rows, int cols, float* col_sum, hipStream_t st) {
    if (rows == 0) return 0;
    const int W = cols * elem_bytes / 4;
    if (W < 1 || W > 256 || (256 % W) != 0) return (int)hipErrorInvalidValue;
    const int rpb = 256 / W;
    int64_t blocks = (rows + rpb - 1) / rpb;
    if (blocks > 1024) blocks = 1024;                            // = nerf_amd_relu_mask_bias_partials() / rpb rows of partial sums
    if (elem_bytes == 2) hipLaunchKernelGGL(relu_mask_bias_kernel<2>, dim3((int)blocks), dim3(256), 0, st, (uint32_t*)delta, (const uint32_t*)act, rows, W, col_sum);
    else hipLaunchKernelGGL(relu_mask_bias_kernel<4>, dim3((int)blocks), dim3(256), 0, st, (uint32_t*)delta, (const uint32_t*)act, rows, W, col_sum);
    return (int)hipGetLastError();
}
int nk::sk_merge_sorted(const float* a, const float* b, int64_t N, int K, int C, float* out, hipStream_t st) {
    if (N == 0) return 0;
    hipLaunchKernelGGL(merge_sorted_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_merge_sorted_lds_bytes(K, C, 0), st, a, b, N, K, C, out);
    return (int)hipGetLastError();
}
int nk::sk_merge_sorted_order(const float* a, const float* b, const int64_t* f_inds, int64_t N, int K, int C, float* out, int64_t* order, int64_t* all_inds,
                          hipStream_t st) {
    if (N == 0) return 0;
    hipLaunchKernelGGL(merge_sorted_order_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), sk_merge_sorted_lds_bytes(K, C, 1), st, a, b, f_inds, N, K, C, out, order, all_inds);
    return (int)hipGetLastError();
}
int nk::sk_coarse_grad_select(const float* grads, const int64_t* sort_inds, int64_t N, int T, int D, int c_pnum, float* out, hipStream_t st) {
    if (N == 0 || c_pnum == 0 || D == 0) return 0;
    hipLaunchKernelGGL(coarse_grad_select_kernel, dim3(blocks_for(N, WAVES_PER_BLOCK)), dim3(256), 0, st, grads, sort_inds, N, T, D, c_pnum, out);
    return (int)hipGetLastError();
}
int nk::sk_weighted_dot_loss(const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* out, float* workspace, hipStream_t st) {
    int64_t nb = (M + 255) / 256;
    const int blocks = (int)(nb > LOSS_BLOCKS ? LOSS_BLOCKS : (nb < 1 ? 1 : nb));
    hipLaunchKernelGGL(weighted_dot_loss_kernel, dim3(blocks), dim3(256), 64, st, w, a, b, M, mode, workspace);
    hipLaunchKernelGGL(weighted_dot_loss_final_kernel, dim3(1), dim3(256), 64, st, workspace, blocks, scale, out);
    return (int)hipGetLastError();
}
int nk::sk_weighted_dot_loss_backward(const float* g, const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* d_w, float* d_a,
                                  float* d_b, hipStream_t st) {
    if (M == 0) return 0;
    hipLaunchKernelGGL(weighted_dot_loss_backward_kernel, dim3(blocks_for(M, 256)), dim3(256), 0, st, g, w, a, b, M, mode, scale, d_w, d_a, d_b);
    return (int)hipGetLastError();
}
// S <= 1024 (checked by the C-ABI): the rows take <= WAVES_PER_BLOCK x 24 x 1023 B = 96 KiB of LDS (mode 0 backward; above the default
// dynamic limit from S = 684 on), the other kernels <= 32 KiB
int nk::sk_distortion_loss(const float* w, const float* t, int64_t N, int S, int mode, float scale, float* out, float* workspace, hipStream_t st) {
    const int M = S - 1;
    int64_t nb = (N + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const int blocks = (int)(nb > DIST_BLOCKS ? DIST_BLOCKS : (nb < 1 ? 1 : nb));
    size_t lds = wave_rows_bytes(dist_wave_floats(2, M));
    if (lds < 64) lds = 64;                                                                  // (the block reduction's 4 x 2 doubles)
    double* partial = reinterpret_cast<double*>(workspace);
    if (mode == 0) hipLaunchKernelGGL(distortion_loss_kernel<0>, dim3(blocks), dim3(256), lds, st, w, t, N, S, partial);
    else hipLaunchKernelGGL(distortion_loss_kernel<1>, dim3(blocks), dim3(256), lds, st, w, t, N, S, partial);
    hipLaunchKernelGGL(distortion_loss_final_kernel, dim3(1), dim3(256), 64, st, partial, blocks, N, M, mode, scale, out);
    return (int)hipGetLastError();
}
int nk::sk_distortion_loss_backward(const float* w, const float* t, int64_t N, int S, int mode, float scale, const float* g, float* d_w, float* d_t,
                                hipStream_t st) {
    if (N == 0 || (!d_w && !d_t)) return 0;
    const size_t lds = wave_rows_bytes(dist_wave_floats(mode == 0 ? 6 : 2, S - 1));
    const dim3 grid(blocks_for(N, WAVES_PER_BLOCK)), block(256);
    if (mode == 0 && lds > 64 * 1024)
        if (int e = nerf_host::allow_dynamic_lds(reinterpret_cast<const void*>(distortion_loss_backward_kernel<0>), lds)) return e;
    if (mode == 0) hipLaunchKernelGGL(distortion_loss_backward_kernel<0>, grid, block, lds, st, w, t, N, S, scale, g, d_w, d_t);
    else hipLaunchKernelGGL(distortion_loss_backward_kernel<1>, grid, block, lds, st, w, t, N, S, scale, g, d_w, d_t);
    return (int)hipGetLastError();
}
// 1 <= M, K <= 1024 (checked by the C-ABI): four waves x <= 16 KiB or two waves x <= 24.6 KB of rows, always within the default 64 KiB
int nk::sk_interlevel_loss(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale, float* out,
                       float* bounds_out, float* workspace, hipStream_t st) {
    const int waves = il_waves(M, K, false);
    int64_t nb = (N + waves - 1) / waves;
    const int blocks = (int)(nb > IL_BLOCKS ? IL_BLOCKS : (nb < 1 ? 1 : nb));
    size_t lds = (size_t)waves * il_wave_bytes(M, K, false);
    if (lds < 64) lds = 64;                                                                  // (the block reduction's doubles)
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(interlevel_loss_kernel, dim3(blocks), dim3(64 * waves), lds, st, w, t, w_prop, t_prop, N, M, K, Kp, partial, bounds_out);
    hipLaunchKernelGGL(interlevel_loss_final_kernel, dim3(1), dim3(256), 64, st, partial, blocks, scale, out);
    return (int)hipGetLastError();
}
int nk::sk_interlevel_loss_backward(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale,
                                const float* g, float* d_w_prop, hipStream_t st) {
    if (N == 0) return 0;
    const int waves = il_waves(M, K, true);
    hipLaunchKernelGGL(interlevel_loss_backward_kernel, dim3(blocks_for(N, waves)), dim3(64 * waves), (size_t)waves * il_wave_bytes(M, K, true), st, w, t,
                       w_prop, t_prop, N, M, K, Kp, scale, g, d_w_prop);
    return (int)hipGetLastError();
}
int nk::sk_encode_rows(const float* x, int x_stride, int64_t M, int L, int normalize, int elem_bytes, void* out, hipStream_t st) {
    if (M == 0) return 0;
    const dim3 grid(blocks_for(M, 256)), block(256);
    char* o = (char*)out;
    if (L == 10 && elem_bytes == 2) hipLaunchKernelGGL((encode_rows_kernel<10, 2>), grid, block, 0, st, x, x_stride, M, normalize, o);
    else if (L == 10) hipLaunchKernelGGL((encode_rows_kernel<10, 4>), grid, block, 0, st, x, x_stride, M, normalize, o);
    else if (L == 4 && elem_bytes == 2) hipLaunchKernelGGL((encode_rows_kernel<4, 2>), grid, block, 0, st, x, x_stride, M, normalize, o);
    else if (L == 4) hipLaunchKernelGGL((encode_rows_kernel<4, 4>), grid, block, 0, st, x, x_stride, M, normalize, o);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
int nk::sk_frag_rows_mask_blocks() { return 512; }                   // partial rows = blocks * WAVES_PER_BLOCK
int nk::sk_frag_rows_mask(const void* frag, int elem_bytes, int64_t n_sub, int n_kg, int64_t M, void* act_out, void* delta, float* col_sum, hipStream_t st) {
    const size_t lds = WAVES_PER_BLOCK * frag_wave_bytes(n_kg, elem_bytes);
    const dim3 grid(sk_frag_rows_mask_blocks()), block(256);     // fixed grid: every wavefront writes its partial row (zeros without work)
    const auto kernel = elem_bytes == 2 ? frag_rows_mask_kernel<2> : frag_rows_mask_kernel<4>;  // (the opt-in below: the fp32 kernel's alone)
    if (int e = elem_bytes == 2 ? 0 : nerf_host::allow_dynamic_lds(reinterpret_cast<const void*>(kernel), 140 * 1024)) return e;
    hipLaunchKernelGGL(kernel, grid, block, lds, st, (const char*)frag, n_sub, n_kg, M, (char*)act_out, (char*)delta, col_sum);
    return (int)hipGetLastError();
}

