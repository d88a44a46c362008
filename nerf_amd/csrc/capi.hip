// extern "C" boundary of libnerf_amd.so (declared in include/nerf_amd.h).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/nerf_amd.h"
#include "mlp_layout.h"

#include "launchers.h"

using namespace nk;

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* a = "") {
    snprintf(g_err, sizeof(g_err), fmt, a);
    return code;
}
int hip_status(int e, const char* where) {
    if (e == 0) return NERF_AMD_OK;
    snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", where, e, hipGetErrorString((hipError_t)e));
    return NERF_AMD_EHIP;
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

int check_samples(const nerf_amd_samples* s, bool need_dir) {
    if (!s) return fail(NERF_AMD_EINVAL, "samples descriptor is NULL");
    if (s->M < 0) return fail(NERF_AMD_EINVAL, "negative sample count");
    if (s->mode == 0) {
        if (!s->pts && s->M) return fail(NERF_AMD_EINVAL, "mode 0 needs pts");
        if (s->pts_stride < (need_dir ? 6 : 3)) return fail(NERF_AMD_EINVAL, "pts_stride too small for this network");
    } else if (s->mode == 1 || s->mode == 2) {
        if (s->S <= 0) return fail(NERF_AMD_EINVAL, "S must be positive");
        if (s->mode == 1 && !s->rays && s->M) return fail(NERF_AMD_EINVAL, "mode 1 needs rays");
        if (s->mode == 2 && (s->H <= 0 || s->W <= 0)) return fail(NERF_AMD_EINVAL, "mode 2 needs H, W");
        if (!s->z && !s->z_base && s->M) return fail(NERF_AMD_EINVAL, "need z, or z_base (with u, or without: in-kernel uniforms from rng_seed)");
    } else {
        return fail(NERF_AMD_EINVAL, "unknown sample mode");
    }
    if (s->contract < 0 || s->contract > NERF_AMD_CONTRACT_GAUSSIAN) return fail(NERF_AMD_EINVAL, "contract must be 0, 1 or NERF_AMD_CONTRACT_GAUSSIAN");
    if (s->ipe) {
        if (!need_dir) return fail(NERF_AMD_EUNSUPPORTED, "integrated PE is wired for the MipNeRF kernel only");
        if (s->mode != 1 || !s->z || s->z_stride < s->S + 1) return fail(NERF_AMD_EINVAL, "integrated PE needs mode 1 with S+1 depths per ray (z, z_stride > S)");
        if (!s->ipe_dir_norm || !(s->ipe_radius > 0.0f)) return fail(NERF_AMD_EINVAL, "integrated PE needs ipe_dir_norm (device) and a positive ipe_radius");
    }
    return NERF_AMD_OK;
}
// a bare descriptor for the MipNeRF network: the Gaussian contraction acts on the frustum of the integrated PE and has no meaning without it
// (the proposal and Ref-NeRF kernels, and the point-encoding passes of a render, read NERF_AMD_CONTRACT_GAUSSIAN as 1)
int check_gaussian(const nerf_amd_samples* s) {
    return (s->contract == NERF_AMD_CONTRACT_GAUSSIAN && !s->ipe) ? fail(NERF_AMD_EINVAL, "contract = NERF_AMD_CONTRACT_GAUSSIAN needs the integrated PE (ipe != 0)") : NERF_AMD_OK;
}
bool bad_prec(int p) { return p != NERF_AMD_F32 && p != NERF_AMD_BF16; }
// layout flags ride above the low byte of a `precision` argument (nerf_amd.h): split them off; true = unknown precision or a flag not in `allowed`
bool split_precision(int& precision, int& lflags, int allowed) {
    lflags = precision & ~0xff;
    precision &= 0xff;
    return bad_prec(precision) || (lflags & ~allowed);
}
// A shape is accepted only if the launch it leads to (launchers.h: sk_*_lds_bytes) fits 64 KiB, the dynamic LDS this project ASSUMES a kernel gets
// without an opt-in (host_common.h).  The assumption is unmeasured: the runtime may well launch more.
int check_lds(size_t bytes, const char* what) {
    return bytes > 64 * 1024 ? fail(NERF_AMD_EINVAL, "%s too large: the per-ray rows of four rays must fit 64 KiB of LDS", what) : NERF_AMD_OK;
}
int check_distortion(int64_t N, int Sn, int mode) {
    if (N < 0) return fail(NERF_AMD_EINVAL, "negative ray count");
    if (mode != 0 && mode != 1) return fail(NERF_AMD_EINVAL, "unknown mode (0: Regularizer, 1: Mip-NeRF 360 L_dist)");
    if (Sn < 2 || Sn > NERF_AMD_DISTORTION_MAX_S) return fail(NERF_AMD_EINVAL, "bad size (S must be 2..1024 depths per row: a ray's rows live in LDS)");
    return NERF_AMD_OK;
}
int check_interlevel(int64_t N, int M, int K, int Kp) {
    if (N < 0) return fail(NERF_AMD_EINVAL, "negative ray count");
    if (M < 1 || M > NERF_AMD_INTERLEVEL_MAX || K < 1 || K > NERF_AMD_INTERLEVEL_MAX)
        return fail(NERF_AMD_EINVAL, "bad size (M and K must be 1..1024 intervals per row: a ray's rows live in LDS)");
    if (Kp != K && Kp != K + 1) return fail(NERF_AMD_EINVAL, "bad size (t_prop has K + 1 edges per row, or K depths: the last interval open)");
    return NERF_AMD_OK;
}
// disparity ray spacing: 0 < near < far, the only kind the warped entry points accept; gn = fp32(1/near), gf = fp32(1/far), each computed in
// double and rounded once
int check_spacing(int spacing, float near, float far, float* gn, float* gf) {
    if (spacing != NERF_AMD_SPACING_DISPARITY) return fail(NERF_AMD_EINVAL, "unknown spacing (the warped entry points take NERF_AMD_SPACING_DISPARITY only)");
    if (!(near > 0.0f)) return fail(NERF_AMD_EINVAL, "disparity spacing needs near > 0");
    if (!(far > near) || !(far <= 3.0e38f)) return fail(NERF_AMD_EINVAL, "disparity spacing needs near < far (finite)");
    *gn = (float)(1.0 / (double)near);
    *gf = (float)(1.0 / (double)far);
    if (!(*gf < *gn)) return fail(NERF_AMD_EINVAL, "disparity spacing: 1/near and 1/far coincide in fp32");
    return NERF_AMD_OK;
}
int check_warped_resample_shape(int C, int K) {
    if (C < 3 || C > 256 || K < 1 || K > 1024) return fail(NERF_AMD_EINVAL, "need 3 <= C <= 256 and 1 <= K <= 1024");
    return check_lds(sk_warped_resample_lds_bytes(C, K), "C and K");
}
}  // namespace

extern "C" {

const char* nerf_amd_last_error(void) { return g_err; }
int nerf_amd_version(void) { return 125; }

int nerf_amd_device_info(int* n_cu, int* arch_is_gfx950) {
    int dev = 0;
    hipDeviceProp_t p;
    int e = (int)hipGetDevice(&dev);
    if (!e) e = (int)hipGetDeviceProperties(&p, dev);
    if (e) return hip_status(e, "nerf_amd_device_info");
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (arch_is_gfx950) *arch_is_gfx950 = strncmp(p.gcnArchName, "gfx950", 6) == 0;
    return NERF_AMD_OK;
}

size_t nerf_amd_packed_bytes(int net, int precision) {
    if (bad_prec(precision)) return 0;
    if (net == NERF_AMD_NET_PROPOSAL) return PropLayout::packed_bytes(precision);
    if (net == NERF_AMD_NET_MIP) return MipLayout::packed_bytes(precision);
    if (net == NERF_AMD_NET_REF) return RefLayout::packed_bytes(precision);
    if (net == NERF_AMD_NET_PROPOSAL_128) return PropLayout128::packed_bytes(precision);
    if (net == NERF_AMD_NET_MIP_128) return MipLayout128::packed_bytes(precision);
    return 0;
}
static int launch_mip_any(int flags, const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, hipStream_t st) {
    return (flags & NERF_AMD_FINE_W128) ? mlp_launch_mip128(packed, precision, s, rgbo, st) : mlp_launch_mip(packed, precision, s, rgbo, st);
}
// the proposal pass of an entry point: `flags` = the layout bits of its precision argument
static int launch_proposal_any(int flags, const void* packed, int precision, const nerf_amd_samples& s, float* density, hipStream_t st) {
    return (flags & NERF_AMD_PROP_W128) ? mlp_launch_proposal128(packed, precision, s, density, st) : mlp_launch_proposal(packed, precision, s, density, st);
}

int nerf_amd_pack_weights(int net, int precision, const float* const* weights, const float* const* biases, int n_tensors,
                          void* packed, void* stream) {
    if (bad_prec(precision)) return fail(NERF_AMD_EINVAL, "unknown precision");
    if (!weights || !biases || !packed) return fail(NERF_AMD_EINVAL, "NULL argument");
    const int want = (net == NERF_AMD_NET_PROPOSAL || net == NERF_AMD_NET_PROPOSAL_128) ? 5
                     : ((net == NERF_AMD_NET_MIP || net == NERF_AMD_NET_MIP_128) ? 11 : (net == NERF_AMD_NET_REF ? 20 : -1));
    if (want < 0) return fail(NERF_AMD_EINVAL, "unknown network");
    if (n_tensors != want) return fail(NERF_AMD_EINVAL, "wrong number of weight tensors for this network");
    for (int i = 0; i < want; ++i)
        if (!weights[i] || !biases[i]) return fail(NERF_AMD_EINVAL, "NULL weight or bias tensor");
    const int e = net == NERF_AMD_NET_PROPOSAL ? pack_proposal(precision, weights, biases, packed, S(stream))
                  : net == NERF_AMD_NET_PROPOSAL_128 ? pack_proposal128(precision, weights, biases, packed, S(stream))
                  : net == NERF_AMD_NET_MIP_128 ? pack_mip128(precision, weights, biases, packed, S(stream))
                  : (net == NERF_AMD_NET_MIP ? pack_mip(precision, weights, biases, packed, S(stream))
                                             : pack_ref(precision, weights, biases, packed, S(stream)));
    return hip_status(e, "nerf_amd_pack_weights");
}

int nerf_amd_proposal_forward(const void* packed, int precision, const nerf_amd_samples* src, float* density, void* stream) {
    int lflags;
    if (split_precision(precision, lflags, NERF_AMD_PROP_W128)) return fail(NERF_AMD_EINVAL, "unknown precision");
    if (int c = check_samples(src, false)) return c;
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !density) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(launch_proposal_any(lflags, packed, precision, *src, density, S(stream)), "nerf_amd_proposal_forward");
}

int nerf_amd_mip_forward(const void* packed, int precision, const nerf_amd_samples* src, float* rgbo, void* stream) {
    int lflags;
    if (split_precision(precision, lflags, NERF_AMD_FINE_W128)) return fail(NERF_AMD_EINVAL, "unknown precision");
    if (int c = check_samples(src, true)) return c;
    if (int c = check_gaussian(src)) return c;
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !rgbo) return fail(NERF_AMD_EINVAL, "NULL argument");
    if ((lflags & NERF_AMD_FINE_W128) && src->ipe) return fail(NERF_AMD_EINVAL, "the 128-wide fine layout has no integrated-PE kernel: pack the network 256-wide");
    return hip_status(launch_mip_any(lflags, packed, precision, *src, rgbo, S(stream)), "nerf_amd_mip_forward");
}

int nerf_amd_direction_table(const float* rays, int64_t N, void* table, void* stream) {
    if (N < 0) return fail(NERF_AMD_EINVAL, "negative ray count");
    if (N && (!rays || !table)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (reinterpret_cast<uintptr_t>(table) & 15) return fail(NERF_AMD_EINVAL, "the table must be 16-byte aligned");
    return hip_status(mlp_launch_dir_table(rays, N, table, S(stream)), "nerf_amd_direction_table");
}

int nerf_amd_mip_forward_composite(const void* packed, int precision, const nerf_amd_samples* src, int white_bkg, float near,
                                   float far, float* rgb, float* depth, float* weights, void* stream) {
    int lflags;
    if (split_precision(precision, lflags, NERF_AMD_FINE_W128)) return fail(NERF_AMD_EINVAL, "unknown precision");
    if (lflags & NERF_AMD_FINE_W128)
        return fail(NERF_AMD_EUNSUPPORTED, "the 128-wide fine layout has no fused-compositing kernel: use nerf_amd_mip_forward + nerf_amd_composite");
    if (int c = check_samples(src, true)) return c;
    if (int c = check_gaussian(src)) return c;
    if (src->mode != 1 || !src->z) return fail(NERF_AMD_EUNSUPPORTED, "fused compositing needs mode 1 (rays + z)");
    if (src->ipe) return fail(NERF_AMD_EUNSUPPORTED, "integrated PE: use nerf_amd_mip_forward + nerf_amd_composite");
    if (src->S != 32 && src->S != 64 && src->S != 128) return fail(NERF_AMD_EUNSUPPORTED, "fused compositing needs S in {32, 64, 128}");
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !rgb) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(mlp_launch_mip_composite(packed, precision, *src, rgb, depth, weights, white_bkg, near, far, S(stream)),
                      "nerf_amd_mip_forward_composite");
}

static bool bad_ref_flags(int f) { return (f & ~NERF_AMD_REF_SRGB) != 0; }
static int ref_forward_any(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, const float* bn_noise, bool train, float* rgbo,
                           float* normal, void* stream, const char* name) {
    if (bad_prec(precision) || bad_ref_flags(ref_flags)) return fail(NERF_AMD_EINVAL, "unknown precision or ref_flags");
    if (int c = check_samples(src, true)) return c;
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !rgbo || (train && !bn_noise)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(mlp_launch_ref(packed, precision, *src, rgbo, normal, bn_noise, ref_flags, S(stream)), name);
}
int nerf_amd_ref_forward(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, float* rgbo, float* normal, void* stream) {
    return ref_forward_any(packed, precision, src, ref_flags, nullptr, false, rgbo, normal, stream, "nerf_amd_ref_forward");
}
int nerf_amd_ref_forward_train(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, const float* bn_noise, float* rgbo,
                               float* normal, void* stream) {
    return ref_forward_any(packed, precision, src, ref_flags, bn_noise, true, rgbo, normal, stream, "nerf_amd_ref_forward_train");
}

int nerf_amd_positional_encoding(const float* x, int64_t M, int L, float* out, void* stream) {
    if (M < 0 || L < 1 || L > 24) return fail(NERF_AMD_EINVAL, "bad M or L");
    if (M && (!x || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_positional_encoding(x, M, L, out, S(stream)), "nerf_amd_positional_encoding");
}

static int ipe_feature_any(const float* z, const float* rays, int64_t N, int Sn, int L, float r, const float* dir_norm, float* feat, float* mu, float* mu_t,
                           int contract, void* stream, const char* name) {
    if (N < 0 || Sn < 0 || L < 1 || L > 15) return fail(NERF_AMD_EINVAL, "bad size or L (1..15)");
    if (N * Sn && (!z || !rays || !dir_norm || !feat)) return fail(NERF_AMD_EINVAL, "NULL argument");
    const float r2 = (float)((double)r * (double)r);        // Python's `r ** 2` is a double, rounded when it meets the fp32 tensor
    return hip_status(sk_ipe_feature(z, rays, N, Sn, L, r2, dir_norm, feat, mu, mu_t, contract, S(stream)), name);
}
int nerf_amd_ipe_feature(const float* z, const float* rays, int64_t N, int Sn, int L, float r, const float* dir_norm, float* feat, float* mu,
                         float* mu_t, void* stream) {
    return ipe_feature_any(z, rays, N, Sn, L, r, dir_norm, feat, mu, mu_t, 0, stream, "nerf_amd_ipe_feature");
}
int nerf_amd_ipe_feature_contracted(const float* z, const float* rays, int64_t N, int Sn, int L, float r, const float* dir_norm, float* feat, float* mu,
                                    float* mu_t, void* stream) {
    return ipe_feature_any(z, rays, N, Sn, L, r, dir_norm, feat, mu, mu_t, 1, stream, "nerf_amd_ipe_feature_contracted");
}
int nerf_amd_ipe_feature_gaussian(const float* z, const float* rays, int64_t N, int Sn, int L, float r, const float* dir_norm, float* feat, float* mu,
                                  float* mu_t, void* stream) {
    return ipe_feature_any(z, rays, N, Sn, L, r, dir_norm, feat, mu, mu_t, NERF_AMD_CONTRACT_GAUSSIAN, stream, "nerf_amd_ipe_feature_gaussian");
}
int nerf_amd_cone_parameters(const float* z, int64_t N, int Sn, float r, float* mu_t, float* var_t, float* var_r, void* stream) {
    if (N < 0 || Sn < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (N * Sn && (!z || !mu_t || !var_t || !var_r)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_cone_parameters(z, N, Sn, (float)((double)r * (double)r), mu_t, var_t, var_r, S(stream)), "nerf_amd_cone_parameters");
}
int nerf_amd_dirs_norm(const float* rays, int64_t N, float* out, void* stream) {
    if (N < 0 || !out || (N && !rays)) return fail(NERF_AMD_EINVAL, "bad argument");
    return hip_status(sk_dirs_norm(rays, N, out, S(stream)), "nerf_amd_dirs_norm");
}

int nerf_amd_generate_rays(const float* pose_host, int H, int W, float fx, float fy, int64_t ray_offset, int64_t N, float* rays,
                           void* stream) {
    if (!pose_host || !rays || H <= 0 || W <= 0) return fail(NERF_AMD_EINVAL, "bad argument");
    if (ray_offset < 0 || N < 0 || ray_offset + N > (int64_t)H * W) return fail(NERF_AMD_EINVAL, "ray range outside the image");
    return hip_status(sk_generate_rays(pose_host, H, W, fx, fy, ray_offset, N, rays, S(stream)), "nerf_amd_generate_rays");
}

// a HOST camera row (nerf_amd.h): finite, fx, fy > 0, reserved tail zero
static int check_camera_row(const char* name, const float* c) {
    if (!c) return fail(NERF_AMD_EINVAL, "%s: camera is NULL", name);
    for (int i = 0; i < NERF_AMD_CAMERA_ROW; ++i)
        if (!(c[i] - c[i] == 0.0f)) return fail(NERF_AMD_EINVAL, "%s: camera has a non-finite value", name);
    if (!(c[0] > 0.0f && c[1] > 0.0f)) return fail(NERF_AMD_EINVAL, "%s: camera needs fx, fy > 0", name);
    for (int i = 9; i < NERF_AMD_CAMERA_ROW; ++i)
        if (c[i] != 0.0f) return fail(NERF_AMD_EINVAL, "%s: camera reserved tail (entries 9..11) must be zero", name);
    return NERF_AMD_OK;
}
int nerf_amd_generate_rays_camera(const float* pose_host, int H, int W, const float* camera_host, int64_t ray_offset, int64_t N, float* rays,
                                  void* stream) {
    const char* name = "nerf_amd_generate_rays_camera";
    if (!pose_host) return fail(NERF_AMD_EINVAL, "%s: pose_host is NULL", name);
    if (!rays) return fail(NERF_AMD_EINVAL, "%s: rays is NULL", name);
    if (H <= 0 || W <= 0) return fail(NERF_AMD_EINVAL, "%s: H, W must be positive", name);
    if (int e = check_camera_row(name, camera_host)) return e;
    if (ray_offset < 0 || N < 0 || ray_offset + N > (int64_t)H * W) return fail(NERF_AMD_EINVAL, "%s: ray range outside the image", name);
    return hip_status(sk_generate_rays_camera(pose_host, H, W, camera_host, ray_offset, N, rays, S(stream)), name);
}

int nerf_amd_length2pts(const float* rays, const float* z, int64_t N, int Sn, float* out, void* stream) {
    if (N < 0 || Sn < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (N * Sn && (!rays || !z || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_length2pts(rays, z, N, Sn, out, S(stream)), "nerf_amd_length2pts");
}

int nerf_amd_sigma_to_weights(const float* sigma, const float* z, const float* dirs, int64_t N, int Sn, int act, float* w,
                              void* stream) {
    if (N < 0 || Sn < 0 || act < 0 || act > 2) return fail(NERF_AMD_EINVAL, "bad size or activation");
    if (N * Sn && (!sigma || !z || !w)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_sigma_to_weights(sigma, z, dirs, N, Sn, act, w, S(stream)), "nerf_amd_sigma_to_weights");
}

int nerf_amd_max_blur(const float* w, int64_t N, int Sn, float alpha, float* out, void* stream) {
    if (N < 0 || Sn < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (N * Sn && (!w || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_max_blur(w, N, Sn, alpha, out, S(stream)), "nerf_amd_max_blur");
}

int nerf_amd_inverse_sample(const float* w, const float* z, const float* u, int64_t N, int C, int K, int sort, float* z_out,
                            int64_t* below, void* stream) {
    if (N < 0 || C < 3 || C > 256 || K < 1 || K > 1024) return fail(NERF_AMD_EINVAL, "need 3 <= C <= 256 and 1 <= K <= 1024");
    if (int e = check_lds(sk_inverse_sample_lds_bytes(C, K), "C and K")) return e;
    if (N && (!w || !z || !u || !z_out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_inverse_sample(w, z, u, N, C, K, sort, 0, z_out, below, nullptr, S(stream)), "nerf_amd_inverse_sample");
}

int nerf_amd_sample_pdf(const float* bins, const float* weights, const float* u, int64_t N, int B, int K, float* samples,
                        int64_t* below, int64_t* above, void* stream) {
    if (N < 0 || B < 2 || B > 256 || K < 1 || K > 1024) return fail(NERF_AMD_EINVAL, "need 2 <= B <= 256 and 1 <= K <= 1024");
    if (int e = check_lds(sk_inverse_sample_lds_bytes(B, K), "B and K")) return e;
    if (N && (!bins || !weights || !u || !samples)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_inverse_sample(weights, bins, u, N, B, K, 0, 1, samples, below, above, S(stream)), "nerf_amd_sample_pdf");
}

int nerf_amd_pixel_rays(const float* pose_host, float fx, float fy, const int64_t* coords, int64_t N, float* rays, void* stream) {
    if (!pose_host || N < 0 || (N && (!coords || !rays))) return fail(NERF_AMD_EINVAL, "bad argument");
    return hip_status(sk_pixel_rays(pose_host, fx, fy, coords, N, rays, S(stream)), "nerf_amd_pixel_rays");
}

// the pose and the seed come from the host (pose_host, rng_seed) or both from the device (pose_dev, seed_dev)
static int train_sampler_any(const float* rgbs, const int64_t* coords, int64_t n_pixels, const float* pose_host, const float* pose_dev, float fx, float fy,
                             float near, float far, int64_t N, int C, uint64_t rng_seed, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb,
                             float* rays, void* stream, const char* name) {
    if (N < 0 || C < 0 || n_pixels < 1) return fail(NERF_AMD_EINVAL, "bad size");
    if (!(pose_host || (pose_dev && seed_dev)) || (N && (!rgbs || !coords || !rgb || !rays))) return fail(NERF_AMD_EINVAL, "NULL argument");
    if ((pts == nullptr) != (lengths == nullptr) || (pts && C < 1)) return fail(NERF_AMD_EINVAL, "pts and lengths go together (C >= 1)");
    return hip_status(sk_train_sampler(rgbs, coords, n_pixels, pose_host, pose_dev, fx, fy, near, far, N, C, rng_seed, seed_dev, pts, lengths, rgb, rays, S(stream)), name);
}
int nerf_amd_sample_training_rays(const float* rgbs, const int64_t* coords, int64_t n_pixels, const float* pose_host, float fx, float fy,
                                  float near, float far, int64_t N, int C, uint64_t rng_seed, float* pts, float* lengths, float* rgb, float* rays,
                                  void* stream) {
    return train_sampler_any(rgbs, coords, n_pixels, pose_host, nullptr, fx, fy, near, far, N, C, rng_seed, nullptr, pts, lengths, rgb, rays, stream,
                             "nerf_amd_sample_training_rays");
}
int nerf_amd_sample_training_rays_dev(const float* rgbs, const int64_t* coords, int64_t n_pixels, const float* pose_dev, float fx, float fy,
                                      float near, float far, int64_t N, int C, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb,
                                      float* rays, void* stream) {
    return train_sampler_any(rgbs, coords, n_pixels, nullptr, pose_dev, fx, fy, near, far, N, C, 0, seed_dev, pts, lengths, rgb, rays, stream,
                             "nerf_amd_sample_training_rays_dev");
}
// the argument checks nerf_amd_sample_scene_rays and its camera twin share (everything but the intrinsics), named for the caller
static int check_scene_sampler(const char* name, const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1,
                               int y0, int y1, int64_t N, int C, const float* pts, const float* lengths, const float* rgb, const float* rays) {
    if (!images) return fail(NERF_AMD_EINVAL, "%s: images is NULL", name);
    if (!poses) return fail(NERF_AMD_EINVAL, "%s: poses is NULL", name);
    if (V < 1 || H < 1 || W < 1) return fail(NERF_AMD_EINVAL, "%s: V, H, W must be positive", name);
    if (K < 1 || (!view_ids && K > V)) return fail(NERF_AMD_EINVAL, "%s: need 1 <= K (and K <= V without view_ids)", name);
    if (x0 < 0 || x1 > W || x0 >= x1) return fail(NERF_AMD_EINVAL, "%s: window x0, x1 empty or outside the image (0 <= x0 < x1 <= W)", name);
    if (y0 < 0 || y1 > H || y0 >= y1) return fail(NERF_AMD_EINVAL, "%s: window y0, y1 empty or outside the image (0 <= y0 < y1 <= H)", name);
    if (N < 0) return fail(NERF_AMD_EINVAL, "%s: N is negative", name);
    if (C < 0) return fail(NERF_AMD_EINVAL, "%s: C is negative", name);
    if (pts && !lengths) return fail(NERF_AMD_EINVAL, "%s: pts given without lengths", name);
    if (lengths && C > 0 && !pts) return fail(NERF_AMD_EINVAL, "%s: lengths given without pts", name);
    if (!rgb) return fail(NERF_AMD_EINVAL, "%s: rgb is NULL", name);
    if (!rays) return fail(NERF_AMD_EINVAL, "%s: rays is NULL", name);
    return NERF_AMD_OK;
}
int nerf_amd_sample_scene_rays(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1,
                               int y0, int y1, float fx, float fy, float near, float far, int64_t N, int C, uint64_t rng_seed,
                               const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index, void* stream) {
    if (int e = check_scene_sampler("nerf_amd_sample_scene_rays", images, poses, V, H, W, view_ids, K, x0, x1, y0, y1, N, C, pts, lengths, rgb, rays)) return e;
    if (N == 0) return NERF_AMD_OK;
    return hip_status(sk_scene_sampler(images, poses, V, H, W, view_ids, K, x0, x1, y0, y1, fx, fy, near, far, N, C, rng_seed, seed_dev, pts, lengths, rgb,
                                       rays, index, S(stream)),
                      "nerf_amd_sample_scene_rays");
}
// the device table's values are the caller's: only the pointer can be checked here
int nerf_amd_sample_scene_rays_camera(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1,
                                      int y0, int y1, const float* cameras, float near, float far, int64_t N, int C, uint64_t rng_seed,
                                      const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index, void* stream) {
    if (int e = check_scene_sampler("nerf_amd_sample_scene_rays_camera", images, poses, V, H, W, view_ids, K, x0, x1, y0, y1, N, C, pts, lengths, rgb, rays)) return e;
    if (!cameras) return fail(NERF_AMD_EINVAL, "nerf_amd_sample_scene_rays_camera: cameras is NULL");
    if (N == 0) return NERF_AMD_OK;
    return hip_status(sk_scene_sampler_camera(images, poses, cameras, V, H, W, view_ids, K, x0, x1, y0, y1, near, far, N, C, rng_seed, seed_dev, pts, lengths,
                                              rgb, rays, index, S(stream)),
                      "nerf_amd_sample_scene_rays_camera");
}
int nerf_amd_philox_uniforms(float* out, int64_t N, int K, uint64_t rng_seed, const uint64_t* seed_dev, void* stream) {
    if (N < 0 || K < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (N * K && !out) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_philox_uniforms(out, N, K, rng_seed, seed_dev, 0, 0, S(stream)), "nerf_amd_philox_uniforms");
}
int nerf_amd_philox_stream(float* out, int64_t N, int K, uint64_t rng_seed, const uint64_t* seed_dev, int64_t ray_offset, int stream_id, void* stream) {
    if (N < 0 || K < 0 || ray_offset < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (stream_id != NERF_AMD_PHILOX_INV && stream_id != NERF_AMD_PHILOX_STRAT) return fail(NERF_AMD_EINVAL, "unknown stream_id");
    if (stream_id == NERF_AMD_PHILOX_STRAT && K > 64) return fail(NERF_AMD_EINVAL, "the stratified stream has 64 slots per ray");
    if (N * K && !out) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_philox_uniforms(out, N, K, rng_seed, seed_dev, ray_offset, stream_id == NERF_AMD_PHILOX_STRAT, S(stream)), "nerf_amd_philox_stream");
}
int nerf_amd_advance_seed(uint64_t* seed_dev, void* stream) {
    if (!seed_dev) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_advance_seed(seed_dev, S(stream)), "nerf_amd_advance_seed");
}

int nerf_amd_stratified_points(const float* rays, const float* z_base, const float* u, float z_jitter, int64_t N, int Sn,
                               float* z_out, float* pts, void* stream) {
    if (N < 0 || Sn < 0) return fail(NERF_AMD_EINVAL, "negative size");
    if (N * Sn && (!z_base || !u || !z_out || (pts && !rays))) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_stratified_points(rays, z_base, u, z_jitter, N, Sn, z_out, pts, S(stream)), "nerf_amd_stratified_points");
}

int nerf_amd_resample(const float* density, const float* z, const float* z_base, const float* u_strat, float z_jitter,
                      const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K, int softplus_density,
                      float blur_alpha, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, int64_t* below, float* w_prop,
                      float* z_coarse, void* stream) {
    if (N < 0 || C < 3 || C > 256 || K < 1 || K > 1024) return fail(NERF_AMD_EINVAL, "need 3 <= C <= 256 and 1 <= K <= 1024");
    if (int e = check_lds(sk_resample_lds_bytes(C, K), "C and K")) return e;   // (5 C + 2 K <= 2816: K <= 768 at C = 256)
    if (N && (!density || !dirs || !z_fine)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (N && !z && !z_base) return fail(NERF_AMD_EINVAL, "need z, or z_base (with u_strat, or without: in-kernel uniforms)");
    return hip_status(sk_resample(density, z, z_base, u_strat, z_jitter, dirs, dirs_stride, u_inv, N, C, K, softplus_density,
                                  blur_alpha, rng_seed, rng_ray_offset, z_fine, below, w_prop, z_coarse, S(stream)), "nerf_amd_resample");
}

int nerf_amd_composite(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int Sn,
                       int flags, int act, float sigma_shift, float near, float far, const float* normal, const float* cam_dir, float* rgb,
                       float* weights, float* depth, float* normal_img, void* stream) {
    if (N < 0 || Sn < 1 || act < 0 || act > 2 || z_stride < Sn) return fail(NERF_AMD_EINVAL, "bad size, stride or activation");
    if (N && (!rgbo || !z || !dirs || !rgb)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (normal_img && !(normal && cam_dir)) return fail(NERF_AMD_EINVAL, "normal_img needs normal and cam_dir");
    return hip_status(sk_composite(rgbo, z, z_stride, dirs, dirs_stride, N, Sn, flags, act, sigma_shift, near, far, normal, cam_dir,
                                   rgb, weights, depth, normal_img, S(stream)), "nerf_amd_composite");
}

int nerf_amd_get_bounds(const float* w_prop, const int64_t* below, int64_t N, int C, int K, float* bounds, void* stream) {
    if (N < 0 || C < 1 || C > 4096 || K < 2) return fail(NERF_AMD_EINVAL, "bad size");
    if (int e = check_lds(sk_get_bounds_lds_bytes(C), "C")) return e;           // (C + 1 floats per ray: C <= 4095)
    if (N && (!w_prop || !below || !bounds)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_get_bounds(w_prop, below, N, C, K, bounds, S(stream)), "nerf_amd_get_bounds");
}

int nerf_amd_merge_depths(const float* z_fine, const float* z_coarse, int64_t N, int K, int C, float* z_out, void* stream) {
    if (N < 0 || K < 1 || C < 1 || sk_merge_sorted_lds_bytes(K, C, 0) > 64 * 1024) return fail(NERF_AMD_EINVAL, "bad size (K + C <= 2048: four rays of depths and their sort scratch per workgroup live in 64 KiB of LDS)");
    if (N && (!z_fine || !z_coarse || !z_out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_merge_sorted(z_fine, z_coarse, N, K, C, z_out, S(stream)), "nerf_amd_merge_depths");
}

int nerf_amd_merge_depths_order(const float* z_fine, const float* z_coarse, const int64_t* f_inds, int64_t N, int K, int C, float* z_out, int64_t* order,
                                int64_t* all_inds, void* stream) {
    if (N < 0 || K < 1 || C < 1 || sk_merge_sorted_lds_bytes(K, C, 1) > 64 * 1024) return fail(NERF_AMD_EINVAL, "bad size (K + C <= 1024: four rays of depths, indices and their sort scratch per workgroup live in 64 KiB of LDS)");
    if (N && (!z_fine || !z_coarse || !z_out || !order)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (N && all_inds && !f_inds) return fail(NERF_AMD_EINVAL, "all_inds needs f_inds");
    return hip_status(sk_merge_sorted_order(z_fine, z_coarse, f_inds, N, K, C, z_out, order, all_inds, S(stream)), "nerf_amd_merge_depths_order");
}

int nerf_amd_coarse_grad_select(const float* grads, const int64_t* sort_inds, int64_t N, int T, int D, int c_pnum, float* out, void* stream) {
    if (N < 0 || T < 1 || D < 1 || c_pnum < 0 || c_pnum > T) return fail(NERF_AMD_EINVAL, "bad size");
    if (N && c_pnum && (!grads || !sort_inds || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_coarse_grad_select(grads, sort_inds, N, T, D, c_pnum, out, S(stream)), "nerf_amd_coarse_grad_select");
}

int nerf_amd_weighted_dot_loss(const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* out, float* workspace, void* stream) {
    if (M < 0 || (mode != 0 && mode != 1)) return fail(NERF_AMD_EINVAL, "bad size / mode");
    if (!out || !workspace || (M && (!w || !a || !b))) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_weighted_dot_loss(w, a, b, M, mode, scale, out, workspace, S(stream)), "nerf_amd_weighted_dot_loss");
}

int nerf_amd_weighted_dot_loss_backward(const float* g, const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* d_w,
                                        float* d_a, float* d_b, void* stream) {
    if (M < 0 || (mode != 0 && mode != 1)) return fail(NERF_AMD_EINVAL, "bad size / mode");
    if (M && (!g || !w || !a || !b)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_weighted_dot_loss_backward(g, w, a, b, M, mode, scale, d_w, d_a, d_b, S(stream)), "nerf_amd_weighted_dot_loss_backward");
}

int nerf_amd_distortion_loss(const float* w, const float* t, int64_t N, int Sn, int mode, float scale, float* out, float* workspace, void* stream) {
    if (int e = check_distortion(N, Sn, mode)) return e;
    if (!out || !workspace || (N && (!w || !t))) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_distortion_loss(w, t, N, Sn, mode, scale, out, workspace, S(stream)), "nerf_amd_distortion_loss");
}

int nerf_amd_distortion_loss_backward(const float* w, const float* t, int64_t N, int Sn, int mode, float scale, const float* g, float* d_w, float* d_t,
                                      void* stream) {
    if (int e = check_distortion(N, Sn, mode)) return e;
    if (N && (!w || !t || !g)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_distortion_loss_backward(w, t, N, Sn, mode, scale, g, d_w, d_t, S(stream)), "nerf_amd_distortion_loss_backward");
}

int nerf_amd_interlevel_loss(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale,
                             float* out, float* bounds_out, float* workspace, void* stream) {
    if (int e = check_interlevel(N, M, K, Kp)) return e;
    if (!out || !workspace || (N && (!w || !t || !w_prop || !t_prop))) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_interlevel_loss(w, t, w_prop, t_prop, N, M, K, Kp, scale, out, bounds_out, workspace, S(stream)), "nerf_amd_interlevel_loss");
}

int nerf_amd_interlevel_loss_backward(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp,
                                      float scale, const float* g, float* d_w_prop, void* stream) {
    if (int e = check_interlevel(N, M, K, Kp)) return e;
    if (N && (!w || !t || !w_prop || !t_prop || !g || !d_w_prop)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_interlevel_loss_backward(w, t, w_prop, t_prop, N, M, K, Kp, scale, g, d_w_prop, S(stream)), "nerf_amd_interlevel_loss_backward");
}

int nerf_amd_mfma_stream(int iters, int workgroups, int mode, float* sink, void* stream) {
    if (iters < 0 || workgroups < 1 || mode < 0 || mode > 3 || !sink) return fail(NERF_AMD_EINVAL, "bad argument");
    return hip_status(pack_mfma_stream(iters, workgroups, mode, sink, S(stream)), "nerf_amd_mfma_stream");
}

// ---- training forward: the MLP kernels also dump their hidden activations ----
static int train_layers(int net) {
    return net == NERF_AMD_NET_PROPOSAL ? PROP_DUMP_SLOTS : (net == NERF_AMD_NET_MIP ? MIP_DUMP_SLOTS : (net == NERF_AMD_NET_REF ? REF_DUMP_SLOTS : 0));
}
static bool bad_train_prec(int p, int net = NERF_AMD_NET_MIP) {           // the fp8-dump mode exists for the proposal and MipNeRF networks
    return p != NERF_AMD_F32 && p != NERF_AMD_BF16 && !(p == NERF_AMD_BF16_F8 && net != NERF_AMD_NET_REF);
}
size_t nerf_amd_train_dump_bytes(int net, int precision, int64_t M) {
    if (M < 0 || !train_layers(net) || bad_train_prec(precision, net)) return 0;
    // activation slots + one ReLU bit per activation: 1 KiB per slot and 32-sample subtile (Ref-NeRF too since round 4)
    const size_t bits = (size_t)train_layers(net) * mlp_train_mask_stride(precision, M);
    return (size_t)train_layers(net) * mlp_train_layer_stride(precision, M) + bits;
}
int nerf_amd_proposal_forward_train(const void* packed, int precision, const nerf_amd_samples* src, float* density, void* dump, void* stream) {
    if (!packed || !src || !dump) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (bad_train_prec(precision)) return fail(NERF_AMD_EINVAL, "bad precision");
    if (src->M && !density) return fail(NERF_AMD_EINVAL, "NULL output");
    if (int c = check_samples(src, false)) return c;
    return hip_status(mlp_launch_proposal_train(packed, precision, *src, density, dump, S(stream)), "nerf_amd_proposal_forward_train");
}
int nerf_amd_mip_forward_train(const void* packed, int precision, const nerf_amd_samples* src, float* rgbo, void* dump, void* stream) {
    if (!packed || !src || !dump) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (bad_train_prec(precision)) return fail(NERF_AMD_EINVAL, "bad precision");
    if (src->M && !rgbo) return fail(NERF_AMD_EINVAL, "NULL output");
    if (int c = check_samples(src, true)) return c;         // (every sample mode, integrated PE and scene contraction included)
    if (int c = check_gaussian(src)) return c;
    return hip_status(mlp_launch_mip_train(packed, precision, *src, rgbo, dump, S(stream)), "nerf_amd_mip_forward_train");
}
int nerf_amd_train_dump_to_rows(const void* dump, int net, int precision, int64_t M, int layer, int n_features, void* out, void* stream) {
    if (M < 0 || layer < 0 || layer >= train_layers(net) || n_features < 16 || n_features > 256 || (n_features & 15))
        return fail(NERF_AMD_EINVAL, "bad layer or feature count");
    if (M && (!dump || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    const size_t stride = mlp_train_layer_stride(precision, M);
    const int elem = precision == NERF_AMD_BF16 ? 2 : 4;
    const int64_t n_sub = (int64_t)(stride / (16 * (size_t)512 * elem));
    return hip_status(sk_frag_to_rows(reinterpret_cast<const char*>(dump) + (size_t)layer * stride, elem, n_sub, n_features / 16, M, out, S(stream)),
                      "nerf_amd_train_dump_to_rows");
}

int64_t nerf_amd_train_dump_rows_mask_partials(void) { return (int64_t)sk_frag_rows_mask_blocks() * 4; }
int nerf_amd_train_dump_rows_mask(const void* dump, int net, int precision, int64_t M, int layer, int n_features, void* act_out, void* delta,
                                  float* col_sum, void* stream) {
    if (M < 0 || layer < 0 || layer >= train_layers(net) || (n_features != 128 && n_features != 256))
        return fail(NERF_AMD_EINVAL, "bad layer or feature count (128 or 256)");
    if (precision != NERF_AMD_F32 && precision != NERF_AMD_BF16) return fail(NERF_AMD_EINVAL, "bad precision");
    if (!col_sum || (M && (!dump || !act_out || !delta))) return fail(NERF_AMD_EINVAL, "NULL argument");
    const size_t stride = mlp_train_layer_stride(precision, M);
    const int elem = precision == NERF_AMD_BF16 ? 2 : 4;
    const int64_t n_sub = (int64_t)(stride / (16 * (size_t)512 * elem));
    return hip_status(sk_frag_rows_mask(reinterpret_cast<const char*>(dump) + (size_t)layer * stride, elem, n_sub, n_features / 16, M, act_out, delta, col_sum,
                                        S(stream)), "nerf_amd_train_dump_rows_mask");
}

int nerf_amd_relu_mask(void* delta, const void* act, int precision, int64_t n, void* stream) {
    if (n < 0 || (precision == NERF_AMD_BF16 && (n & 1))) return fail(NERF_AMD_EINVAL, "bad element count (bf16: even)");
    if (n && (!delta || !act)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_relu_mask(delta, act, precision == NERF_AMD_BF16 ? 2 : 4, n, S(stream)), "nerf_amd_relu_mask");
}

int64_t nerf_amd_relu_mask_bias_partials(int precision, int64_t rows, int cols) {
    const int W = cols * (precision == NERF_AMD_BF16 ? 2 : 4) / 4;
    if (rows <= 0 || W < 1 || W > 256 || (256 % W) != 0) return 0;
    const int rpb = 256 / W;
    int64_t blocks = (rows + rpb - 1) / rpb;
    if (blocks > 1024) blocks = 1024;
    return blocks * rpb;
}
int nerf_amd_relu_mask_bias(void* delta, const void* act, int precision, int64_t rows, int cols, float* col_sum, void* stream) {
    if (rows < 0 || cols < 2 || (precision != NERF_AMD_F32 && precision != NERF_AMD_BF16)) return fail(NERF_AMD_EINVAL, "bad size or precision");
    if (rows && (!delta || !act || !col_sum)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_relu_mask_bias(delta, act, precision == NERF_AMD_BF16 ? 2 : 4, rows, cols, col_sum, S(stream)), "nerf_amd_relu_mask_bias");
}

int nerf_amd_encode_rows(const float* x, int x_stride, int64_t M, int L, int normalize, int precision, void* out, void* stream) {
    if (M < 0 || x_stride < 3 || (L != 4 && L != 10) || (precision != NERF_AMD_F32 && precision != NERF_AMD_BF16)) return fail(NERF_AMD_EINVAL, "bad size, L (4 or 10) or precision");
    if (M && (!x || !out)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_encode_rows(x, x_stride, M, L, normalize, precision == NERF_AMD_BF16 ? 2 : 4, out, S(stream)), "nerf_amd_encode_rows");
}

// ---- backward of the MLPs: dgrad chain on transposed packed weights, MFMA weight gradients, Adam (bwd_kernels.hip) ----
size_t nerf_amd_packed_backward_bytes(int net, int precision) {
    if (bad_prec(precision)) return 0;
    if (net == NERF_AMD_NET_PROPOSAL) return PropBwdLayout::packed_bytes(precision);
    if (net == NERF_AMD_NET_MIP) return MipBwdLayout::packed_bytes(precision);
    if (net == NERF_AMD_NET_REF) return RefBwdLayout::packed_bytes(precision);
    return 0;
}
int nerf_amd_pack_weights_backward(int net, int precision, const float* const* weights, int n_tensors, void* packed_bwd, void* stream) {
    if (bad_prec(precision)) return fail(NERF_AMD_EINVAL, "unknown precision");
    if (!weights || !packed_bwd) return fail(NERF_AMD_EINVAL, "NULL argument");
    const int want = (net == NERF_AMD_NET_PROPOSAL || net == NERF_AMD_NET_PROPOSAL_128) ? 5 : (net == NERF_AMD_NET_MIP ? 11 : (net == NERF_AMD_NET_REF ? 20 : -1));
    if (want < 0) return fail(NERF_AMD_EINVAL, "unknown network");
    if (n_tensors != want) return fail(NERF_AMD_EINVAL, "wrong number of weight tensors for this network");
    for (int i = 0; i < want; ++i)
        if (!weights[i]) return fail(NERF_AMD_EINVAL, "NULL weight tensor");
    const int e = net == NERF_AMD_NET_PROPOSAL ? pack_proposal_bwd(precision, weights, packed_bwd, S(stream))
                  : (net == NERF_AMD_NET_MIP ? pack_mip_bwd(precision, weights, packed_bwd, S(stream)) : pack_ref_bwd(precision, weights, packed_bwd, S(stream)));
    return hip_status(e, "nerf_amd_pack_weights_backward");
}
int nerf_amd_proposal_backward_chain(const void* packed_bwd, int precision, const float* g_density, int64_t M, const void* act_dump,
                                     void* delta_dump, void* stream) {
    if (bad_train_prec(precision) || M < 0) return fail(NERF_AMD_EINVAL, "bad precision or size");
    if (M == 0) return NERF_AMD_OK;
    if (!packed_bwd || !g_density || !act_dump || !delta_dump) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_launch_prop_chain(packed_bwd, precision, g_density, M, act_dump, delta_dump, S(stream)), "nerf_amd_proposal_backward_chain");
}
int nerf_amd_mip_backward_chain(const void* packed_bwd, int precision, const float* g_rgbo, const float* rgbo, int64_t M, const void* act_dump,
                                void* delta_dump, void* stream) {
    if (bad_train_prec(precision) || M < 0) return fail(NERF_AMD_EINVAL, "bad precision or size");
    if (M == 0) return NERF_AMD_OK;
    if (!packed_bwd || !g_rgbo || !rgbo || !act_dump || !delta_dump) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_launch_mip_chain(packed_bwd, precision, g_rgbo, rgbo, M, act_dump, delta_dump, S(stream)), "nerf_amd_mip_backward_chain");
}
size_t nerf_amd_weight_grads_workspace_bytes(int net, int precision, int64_t M) {
    if (bad_train_prec(precision, net) || M < 0) return 0;
    return bwd_wgrad_workspace_bytes(net, precision == NERF_AMD_BF16_F8 ? NERF_AMD_BF16 : precision, M);
}
int nerf_amd_proposal_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, float* const* d_weights,
                                   float* const* d_biases, void* workspace, void* stream) {
    if (bad_train_prec(precision) || M < 0) return fail(NERF_AMD_EINVAL, "bad precision or size");
    if (!d_weights || !d_biases) return fail(NERF_AMD_EINVAL, "NULL argument");
    for (int i = 0; i < 5; ++i)
        if (!d_weights[i] || !d_biases[i]) return fail(NERF_AMD_EINVAL, "NULL gradient tensor");
    if (M == 0) return fail(NERF_AMD_EINVAL, "no samples (the caller zero-fills the gradients of an empty batch)");
    if (!act_dump || !delta_dump || !workspace) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_prop_weight_grads(precision, M, act_dump, delta_dump, d_weights, d_biases, workspace, S(stream)), "nerf_amd_proposal_weight_grads");
}
int nerf_amd_mip_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, const float* const* weights,
                              const float* const* biases, float* const* d_weights, float* const* d_biases, void* workspace, void* stream) {
    if (bad_train_prec(precision) || M < 0) return fail(NERF_AMD_EINVAL, "bad precision or size");
    if (!weights || !biases || !d_weights || !d_biases) return fail(NERF_AMD_EINVAL, "NULL argument");
    for (int i = 0; i < 11; ++i)
        if (!weights[i] || !biases[i] || !d_weights[i] || !d_biases[i]) return fail(NERF_AMD_EINVAL, "NULL tensor");
    if (M == 0) return fail(NERF_AMD_EINVAL, "no samples (the caller zero-fills the gradients of an empty batch)");
    if (!act_dump || !delta_dump || !workspace) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_mip_weight_grads(precision, M, act_dump, delta_dump, weights, biases, d_weights, d_biases, workspace, S(stream)),
                      "nerf_amd_mip_weight_grads");
}
int nerf_amd_ref_forward_train_dump(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, const float* bn_noise, float* rgbo,
                                    float* normal, void* dump, float* aux, void* stream) {
    if (bad_prec(precision) || bad_ref_flags(ref_flags)) return fail(NERF_AMD_EINVAL, "unknown precision or ref_flags");
    if (int c = check_samples(src, true)) return c;
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !rgbo || !dump || !aux) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(mlp_launch_ref_train(packed, precision, *src, rgbo, normal, bn_noise, dump, aux, ref_flags, S(stream), 0, nullptr, 0.0f), "nerf_amd_ref_forward_train_dump");
}
int nerf_amd_ref_forward_train_dump_rng(const void* packed, int precision, const nerf_amd_samples* src, int ref_flags, uint64_t noise_seed,
                                        const uint64_t* noise_seed_dev, float noise_std, float* rgbo, float* normal, void* dump, float* aux, void* stream) {
    if (bad_prec(precision) || bad_ref_flags(ref_flags)) return fail(NERF_AMD_EINVAL, "unknown precision or ref_flags");
    if (!(noise_std >= 0.0f)) return fail(NERF_AMD_EINVAL, "noise_std must be >= 0");
    if (int c = check_samples(src, true)) return c;
    if (src->M == 0) return NERF_AMD_OK;
    if (!packed || !rgbo || !dump || !aux) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(mlp_launch_ref_train(packed, precision, *src, rgbo, normal, nullptr, dump, aux, ref_flags, S(stream), noise_seed,
                                           reinterpret_cast<const unsigned long long*>(noise_seed_dev), noise_std), "nerf_amd_ref_forward_train_dump_rng");
}
int nerf_amd_philox_normal(float* out, int64_t M, uint64_t rng_seed, const uint64_t* seed_dev, float std, int64_t sample_offset, void* stream) {
    if (M < 0 || sample_offset < 0 || !(std >= 0.0f)) return fail(NERF_AMD_EINVAL, "negative size or std");
    if (M && !out) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_philox_normal(out, M, rng_seed, seed_dev, std, sample_offset, S(stream)), "nerf_amd_philox_normal");
}
size_t nerf_amd_density_grad_workspace_bytes(int net, int precision, int64_t M) {
    if (bad_prec(precision) || M < 0 || (net != NERF_AMD_NET_PROPOSAL && net != NERF_AMD_NET_REF)) return 0;
    return bwd_density_grad_workspace_bytes(precision, M);
}
int nerf_amd_density_grad(int net, const void* packed_bwd, int precision, int64_t M, const void* act_dump, const float* x, int x_stride,
                          const float* scale, int scale_stride, float* grad, void* workspace, void* stream) {
    const int contract = (net & NERF_AMD_CONTRACTED) ? 1 : 0;   // flag in `net`: the forward saw contracted positions (nerf_amd_samples.contract)
    net &= ~NERF_AMD_CONTRACTED;
    if (bad_prec(precision) || M < 0 || x_stride < 3) return fail(NERF_AMD_EINVAL, "bad precision, size or stride");
    if (net != NERF_AMD_NET_PROPOSAL && net != NERF_AMD_NET_REF) return fail(NERF_AMD_EUNSUPPORTED, "density gradients exist for the proposal and Ref-NeRF networks");
    if (M == 0) return NERF_AMD_OK;
    if (!packed_bwd || !act_dump || !x || !grad || !workspace) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_density_grad(net, packed_bwd, precision, M, act_dump, x, x_stride, scale, scale_stride, grad, workspace, S(stream), contract), "nerf_amd_density_grad");
}
size_t nerf_amd_ref_backward_workspace_bytes(int precision, int64_t M) {
    if (bad_prec(precision) || M < 0) return 0;
    return bwd_ref_workspace_bytes(precision, M);
}
int nerf_amd_ref_backward(const void* packed_bwd, int precision, int ref_flags, int64_t M, const void* act_dump, const float* aux, const float* dirs,
                          int dir_stride, const float* g_out, int g_stride, const float* ide_table, float* const* d_weights, float* const* d_biases,
                          void* workspace, void* stream) {
    if (bad_prec(precision) || bad_ref_flags(ref_flags) || M < 0 || dir_stride < 3 || g_stride < 7) return fail(NERF_AMD_EINVAL, "bad precision, flags, size or stride");
    if (!d_weights || !d_biases) return fail(NERF_AMD_EINVAL, "NULL argument");
    for (int i = 0; i < 20; ++i)
        if (!d_weights[i] || !d_biases[i]) return fail(NERF_AMD_EINVAL, "NULL gradient tensor");
    if (M == 0) return fail(NERF_AMD_EINVAL, "no samples (the caller zero-fills the gradients of an empty batch)");
    if (!packed_bwd || !act_dump || !aux || !dirs || !g_out || !ide_table || !workspace) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(bwd_ref_backward(packed_bwd, precision, M, act_dump, aux, dirs, dir_stride, g_out, g_stride, ide_table, d_weights, d_biases, workspace,
                                       ref_flags, S(stream)), "nerf_amd_ref_backward");
}

int nerf_amd_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel,
                       int n_tensors, float* step, double lr, const double* lr_dev, double beta1, double beta2, double eps, float grad_scale,
                       void* stream) {
    if (n_tensors < 0 || (n_tensors && (!params || !grads || !exp_avg || !exp_avg_sq || !numel)) || !step) return fail(NERF_AMD_EINVAL, "NULL argument");
    for (int i = 0; i < n_tensors; ++i)
        if (numel[i] < 0 || (numel[i] && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i]))) return fail(NERF_AMD_EINVAL, "NULL tensor");
    static_assert(sizeof(long long) == sizeof(int64_t), "int64");
    return hip_status(bwd_launch_adam(params, grads, exp_avg, exp_avg_sq, reinterpret_cast<const long long*>(numel), n_tensors, step, lr, lr_dev,
                                      beta1, beta2, eps, grad_scale, S(stream)), "nerf_amd_adam_step");
}

// ---- backward of the sampling / compositing rows ----
int nerf_amd_sigma_to_weights_backward(const float* sigma, const float* z, const float* dirs, int64_t N, int Sn, int act,
                                       const float* d_weights, float* d_sigma, void* stream) {
    if (N < 0 || Sn < 1 || Sn > 1024) return fail(NERF_AMD_EINVAL, "bad size (S must be 1..1024)");
    if (N && (!sigma || !z || !d_weights || !d_sigma)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_weights_backward(sigma, 1, 0, z, Sn, dirs, 3, N, Sn, dirs ? 1 : 0, act, 0.0f, nullptr, nullptr, d_weights, nullptr, 0, 0.0f,
                                          1.0f, d_sigma, 1, 0, nullptr, S(stream)), "nerf_amd_sigma_to_weights_backward");
}
int nerf_amd_composite_backward(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int Sn,
                                int flags, int act, float sigma_shift, float near, float far, const float* d_rgb,
                                const float* d_weights, const float* d_depth, float* d_rgbo, void* stream) {
    if (N < 0 || Sn < 1 || Sn > 1024 || z_stride < Sn) return fail(NERF_AMD_EINVAL, "bad size (S must be 1..1024)");
    if (N && (!rgbo || !z || !dirs || !d_rgbo)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (N && !d_rgb) return fail(NERF_AMD_EINVAL, "d_rgb is required (pass zeros when only the weights carry a gradient)");
    return hip_status(sk_weights_backward(rgbo, 4, 3, z, z_stride, dirs, dirs_stride, N, Sn, flags & 1, act, sigma_shift, rgbo, d_rgb, d_weights,
                                          d_depth, (flags >> 1) & 1, near, far, d_rgbo, 4, 3, d_rgbo, S(stream)), "nerf_amd_composite_backward");
}
int nerf_amd_max_blur_backward(const float* weights, const float* d_out, int64_t N, int Sn, float* d_weights, void* stream) {
    if (N < 0 || Sn < 1) return fail(NERF_AMD_EINVAL, "bad size");
    if (N && (!weights || !d_out || !d_weights)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_max_blur_backward(weights, d_out, N, Sn, d_weights, S(stream)), "nerf_amd_max_blur_backward");
}
int nerf_amd_get_bounds_backward(const int64_t* below, const float* d_bounds, int64_t N, int C, int K, float* d_w_prop, void* stream) {
    if (N < 0 || C < 1 || C > 4096 || K < 2 || sk_get_bounds_backward_lds_bytes(K) > 64 * 1024) return fail(NERF_AMD_EINVAL, "bad size (C <= 4096, 2 <= K <= 2048)");
    if (N && (!below || !d_bounds || !d_w_prop)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_get_bounds_backward(below, d_bounds, N, C, K, d_w_prop, S(stream)), "nerf_amd_get_bounds_backward");
}

// ------------------------------------------------------------------------------------------------ whole-ray rendering
namespace {
constexpr int RENDER_C = 64;                                // procedures.py:22 RENDER_COARSE_PNUM
// The workspace of the four render entry points, described ONCE and selected by what varies -- disparity spacing, a second proposal round
// of P = prop_pnum depths (0: one round), the Ref-NeRF tail: the constructor walks the parts in order, each rounded up to 256 bytes.
// Walked from NULL it gives the size (nerf_amd_render*_workspace_bytes), from the caller's pointer the parts.
//   density (N,64) [| s_c (N,64) | z_c (N,64), warped] [| density2 (N,P) | z_mid (N,P) [| s_mid (N,P), warped], two rounds] | z_fine (N, n_fine+1)
//   MipNeRF:  | rgbo (N, n_fine, 4) [| raw depth (N), warped] | rays (N, 6) | one scalar slot (direction norm of the IPE mode)
//   Ref-NeRF: | z_coarse (N,64) | z_all (N, n_fine+64) | rgbo (N, n_fine+64, 4) | normals (N, n_fine+64, 3) | rays (unrounded)
struct RenderWs {
    float *density, *s_c = nullptr, *z_c = nullptr, *density2 = nullptr, *z_mid = nullptr, *s_mid = nullptr, *z_fine, *z_coarse = nullptr, *z_all = nullptr, *rgbo,
          *normals = nullptr, *depth_raw = nullptr, *rays, *dir_norm;
    size_t bytes;
    RenderWs(bool warped, int prop_pnum, bool ref, void* base, int64_t N, int n_fine) {
        const uintptr_t start = (reinterpret_cast<uintptr_t>(base) + 255) & ~(uintptr_t)255;
        uintptr_t p = start;
        auto take = [&p](size_t part) { float* r = reinterpret_cast<float*>(p); p += (part + 255) & ~(size_t)255; return r; };
        const size_t n = (size_t)N, S = (size_t)n_fine + (ref ? RENDER_C : 0);    // samples per ray of the fine pass
        density = take(n * RENDER_C * 4);
        if (warped) { s_c = take(n * RENDER_C * 4); z_c = take(n * RENDER_C * 4); }
        if (prop_pnum) { density2 = take(n * prop_pnum * 4); z_mid = take(n * prop_pnum * 4); }
        if (prop_pnum && warped) s_mid = take(n * prop_pnum * 4);
        z_fine = take(n * (n_fine + 1) * 4);
        if (ref) { z_coarse = take(n * RENDER_C * 4); z_all = take(n * S * 4); }
        rgbo = take(n * S * 16);
        if (ref) normals = take(n * S * 12);
        if (warped) depth_raw = take(n * 4);
        rays = ref ? reinterpret_cast<float*>(p) : take(n * 24);   // ref: the ray table is the unrounded tail
        dir_norm = reinterpret_cast<float*>(p);             // MipNeRF: the scalar slot behind the ray table
        bytes = (size_t)(p - start) + (ref ? n * 24 + 256 : 512);   // + alignment slack (+ the scalar slot)
    }
};
size_t render_ws_bytes(bool warped, bool ref, int64_t N, int n_fine) { return (N < 0 || n_fine < 1) ? 0 : RenderWs(warped, 0, ref, nullptr, N, n_fine).bytes; }

// One call of any of the four entry points.  The MipNeRF pipeline (render_mip) is: ray table -> direction norm (IPE) -> coarse draw +
// proposal pass -> resampling [-> second proposal pass -> second resampling] -> fine pass -> compositing [-> depth un-warp]; an entry point
// fixes `warped`, `prop_pnum` and where the uniforms come from.  Ref-NeRF shares everything up to the first resampling.
struct RenderPlan {
    const void *packed_prop, *packed_fine;
    int precision, lflags;                                  // lflags: the layout bits, split off `precision` by check_plan_shape
    const float* rays;
    const nerf_amd_samples* camera;
    int64_t ray_offset;
    const float *z_base, *u_strat, *u_inv;                  // z_base: linear spacing only; u_* = NULL: Philox streams of (seed(), ray + ray0())
    int64_t N;
    int n_fine, prop_pnum;                                  // prop_pnum = 0: one proposal round
    bool warped, ref;
    float near, far, gn, gf;                                // gn, gf: check_spacing (warped)
    int white_bkg;
    float *rgb, *depth, *weights;
    // Ref-NeRF only (weights: (N, n_fine + 64) there, reachable through nerf_amd_render alone)
    int ref_flags = 0;
    const float* cam_dir = nullptr;
    float* normal_img = nullptr;
    // nerf_amd_render only: depth quantiles, opacity and the fine depth row (all NULL / 0: the call is the plain entry point)
    float *opacity = nullptr, *depth_q = nullptr, *fine_depths = nullptr;
    float quantiles[NERF_AMD_DEPTH_QUANTILES_MAX] = {0.0f, 0.0f, 0.0f, 0.0f};
    int n_quantiles = 0;
    // nerf_amd_render only: the empty-ray skip (include/nerf_amd.h); off unless skip_dmin > 0
    double skip_dmin = 0.0;
    int32_t* row_of_ray = nullptr;
    int64_t* n_alive = nullptr;
    bool skip() const { return skip_dmin > 0.0; }
    bool skip_stores_coarse() const { return skip() && !ref && !warped && !prop_pnum; }     // the one route whose coarse depths exist in no buffer
    int fine_row() const { return fine_samples() + (ref ? 0 : 1); }        // floats of the depth row the fine pass reads: z_fine, Ref-NeRF z_all
    bool want_stats() const { return opacity || (depth_q && n_quantiles); }
    int fine_samples() const { return n_fine + (ref ? RENDER_C : 0); }      // samples per ray of the fine pass
    bool ipe() const { return !ref && camera && camera->ipe; }
    uint64_t seed() const { return camera ? camera->rng_seed : 0; }     // (read only when a uniform tensor is NULL)
    int64_t ray0() const { return camera ? camera->rng_ray_offset : 0; }
    RenderWs ws(void* base) const { return RenderWs(warped, prop_pnum, ref, base, N, n_fine); }
};
// What nerf_amd_render appends BEHIND the entry point's workspace (whose layout and size query stay): the weights the stats kernel reads
// when the caller takes none, and the raw quantile depths that the un-warp reads under disparity spacing; each rounded up to 256 bytes.
// Behind those, with the empty-ray skip on: row_of_ray (N) int32 | ray_of_row (N) int64 | the device count | flags and tile counts
// (sk_ray_alive_workspace_bytes) | the compact ray table (N,6) | the compact fine depth rows (N, fine_row) [| the coarse depths (N,64) of
// the linear one-round route, which has them in no other buffer].
struct RenderExtrasWs {
    float *weights = nullptr, *depth_q_raw = nullptr;
    int32_t* row_of_ray = nullptr;
    int64_t *ray_of_row = nullptr, *count = nullptr;
    void* alive_ws = nullptr;
    float *rays_c = nullptr, *z_rows_c = nullptr, *z_coarse = nullptr;
    size_t bytes;                                           // of the whole workspace, the entry point's part included
    RenderExtrasWs(const RenderPlan& p, void* base) {
        const RenderWs ws = p.ws(base);
        const size_t n = (size_t)p.N;
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const bool skip = p.skip();
        const size_t parts[9] = {(p.want_stats() && !p.weights) ? up(n * p.fine_samples() * 4) : 0,
                                 (p.warped && p.depth_q && p.n_quantiles) ? up(n * p.n_quantiles * 4) : 0,
                                 skip ? up(n * 4) : 0, skip ? up(n * 8) : 0, skip ? (size_t)256 : 0, skip ? up(sk_ray_alive_workspace_bytes(p.N)) : 0,
                                 skip ? up(n * 24) : 0, skip ? up(n * p.fine_row() * 4) : 0, p.skip_stores_coarse() ? up(n * RENDER_C * 4) : 0};
        size_t sum = 0;
        for (size_t part : parts) sum += part;
        bytes = ws.bytes;
        if (!sum) return;
        const size_t own = (ws.bytes + 255) & ~(size_t)255;    // ws.bytes counts from the caller's pointer, the parts from the aligned start: past its end
        char* at = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 255) & ~(uintptr_t)255) + own;
        auto take = [&at](size_t part) { char* r = part ? at : nullptr; at += part; return r; };
        weights = reinterpret_cast<float*>(take(parts[0]));
        depth_q_raw = reinterpret_cast<float*>(take(parts[1]));
        row_of_ray = reinterpret_cast<int32_t*>(take(parts[2]));
        ray_of_row = reinterpret_cast<int64_t*>(take(parts[3]));
        count = reinterpret_cast<int64_t*>(take(parts[4]));
        alive_ws = take(parts[5]);
        rays_c = reinterpret_cast<float*>(take(parts[6]));
        z_rows_c = reinterpret_cast<float*>(take(parts[7]));
        z_coarse = reinterpret_cast<float*>(take(parts[8]));
        bytes = own + sum + 256;
    }
};
int check_quantiles(const float* q, int nq) {
    if (nq < 0 || nq > NERF_AMD_DEPTH_QUANTILES_MAX) return fail(NERF_AMD_EINVAL, "n_quantiles must be 0..NERF_AMD_DEPTH_QUANTILES_MAX (4)");
    if (nq && !q) return fail(NERF_AMD_EINVAL, "NULL argument: quantiles");
    for (int j = 0; j < nq; ++j)
        if (!(q[j] > 0.0f && q[j] < 1.0f)) return fail(NERF_AMD_EINVAL, "a quantile must lie in (0, 1)");
    return NERF_AMD_OK;
}

// ---- the checks: everything is refused here, before the first launch ----
// what must hold even for N == 0: precision and layout bits, sizes, and that every resampling launch fits the LDS
int check_plan_shape(RenderPlan& p, int layouts, const char* bad_precision) {
    if (split_precision(p.precision, p.lflags, layouts)) return fail(NERF_AMD_EINVAL, bad_precision);
    if ((p.lflags & NERF_AMD_FINE_W128) && p.ipe()) return fail(NERF_AMD_EINVAL, "the 128-wide fine layout has no integrated-PE kernel: pack the network 256-wide");
    if (p.skip() && p.N > 0x7fffffff) return fail(NERF_AMD_EINVAL, "the empty-ray skip indexes rays in int32: N must be below 2^31");
    if (p.N < 0 || p.n_fine < 1 || p.n_fine > 1023) return fail(NERF_AMD_EINVAL, "bad N or n_fine");
    if (p.camera && (p.camera->contract < 0 || p.camera->contract > NERF_AMD_CONTRACT_GAUSSIAN)) return fail(NERF_AMD_EINVAL, "contract must be 0, 1 or NERF_AMD_CONTRACT_GAUSSIAN");
    if (p.camera && !p.ref && p.camera->contract == NERF_AMD_CONTRACT_GAUSSIAN && !p.camera->ipe)
        return fail(NERF_AMD_EINVAL, "contract = NERF_AMD_CONTRACT_GAUSSIAN needs the integrated PE (camera->ipe != 0)");
    const int K = p.n_fine + 1, K1 = p.prop_pnum ? p.prop_pnum : K;                  // depths drawn by the first resampling
    if (int e = p.warped ? check_warped_resample_shape(RENDER_C, K1) : check_lds(sk_resample_lds_bytes(RENDER_C, K1), "prop_pnum")) return e;
    return p.prop_pnum ? check_lds(sk_resample_window_lds_bytes(p.prop_pnum, K, p.warped ? 1 : 0), "prop_pnum and n_fine") : NERF_AMD_OK;
}
// what a call with rays to render needs: its pointers, a source of rays and of uniforms, a usable IPE descriptor
int check_plan_inputs(const RenderPlan& p, const void* workspace) {
    if (!(p.packed_prop && p.packed_fine && (p.warped || p.z_base) && p.rgb && workspace)) return fail(NERF_AMD_EINVAL, "NULL argument");
    if ((p.u_strat == nullptr) != (p.u_inv == nullptr)) return fail(NERF_AMD_EINVAL, "u_strat and u_inv are both given or both NULL (in-kernel uniforms)");
    if (!p.u_strat && !p.camera) return fail(NERF_AMD_EINVAL, "in-kernel uniforms need the descriptor (rng_seed, rng_ray_offset)");
    if (!p.rays && !p.camera) return fail(NERF_AMD_EINVAL, "need rays or camera");
    if (p.warped && p.ipe() && !p.rays) return fail(NERF_AMD_EINVAL, "integrated PE needs an explicit ray table");
    if (!p.rays && (p.camera->H <= 0 || p.camera->W <= 0 || p.ray_offset < 0 || p.ray_offset + p.N > (int64_t)p.camera->H * p.camera->W))
        return fail(NERF_AMD_EINVAL, "ray range outside the camera image");
    if (p.ipe() && !(p.camera->ipe_radius > 0.0f)) return fail(NERF_AMD_EINVAL, "integrated PE needs a positive ipe_radius");
    return NERF_AMD_OK;
}

// ---- the stages: each exists once ----
// row 1 (procedures.py:43-51,64): without a ray table, the camera's rays ray_offset .. ray_offset + N - 1 are generated into the workspace
int provide_rays(const RenderPlan& p, const RenderWs& ws, hipStream_t st, const float** rays) {
    *rays = p.rays ? p.rays : ws.rays;
    if (p.rays) return NERF_AMD_OK;
    const nerf_amd_samples* c = p.camera;
    return hip_status(sk_generate_rays(c->pose, c->H, c->W, c->fx, c->fy, p.ray_offset, p.N, ws.rays, st), "ray generation");
}
// row 12 inside the fine pass (IPE mode; else *dir_norm = NULL): the direction norm of this ray batch, into the workspace's scalar slot (the
// density buffer is free until the proposal pass writes it: room for the 256 fp64 workgroup partials when N >= 8).  A caller that renders a
// SHARD of a ray list hands over the norm of the whole list (camera->ipe_dir_norm): mip_methods.py:31 norms all rays of the reference's call.
int provide_dir_norm(const RenderPlan& p, const float* rays, const RenderWs& ws, hipStream_t st, const float** dir_norm) {
    *dir_norm = !p.ipe() ? nullptr : (p.camera->ipe_dir_norm ? p.camera->ipe_dir_norm : ws.dir_norm);
    if (*dir_norm != ws.dir_norm) return NERF_AMD_OK;
    return hip_status((p.N >= 8) ? sk_dirs_norm_scratch(rays, p.N, ws.dir_norm, ws.density, st) : sk_dirs_norm(rays, p.N, ws.dir_norm, st), "direction norm");
}
// S samples per ray at the depths z (row stride z_stride); the descriptor may accompany explicit rays just to carry `contract`
nerf_amd_samples ray_samples(const RenderPlan& p, const float* rays, int S, const float* z, int z_stride, int64_t n_rays = -1) {    // n_rays < 0: all of the plan's
    nerf_amd_samples s{};
    s.mode = 1; s.rays = rays; s.S = S; s.M = (n_rays < 0 ? p.N : n_rays) * S; s.z = z; s.z_stride = z_stride; s.contract = p.camera ? p.camera->contract : 0;
    return s;
}
// rows 2-7: the coarse draw and the proposal pass, then weights -> max-blur(0.01) -> inverse sampling of K sorted depths into z_out
// (procedures.py:59,68-70).  Linear spacing: the stratified z is fused into the proposal MLP, and ws.z_coarse (Ref-NeRF) also receives the
// depths it used.  Disparity spacing: the draw happens in s (no position tensor: the proposal MLP forms o + z d itself), s_out receives the
// resampled s next to z_out = W(s).  z_coarse (linear spacing; may be NULL): receives the coarse depths the resampling kernel drew.
int coarse_pass(const RenderPlan& p, const float* rays, int K, float* z_out, float* s_out, float* z_coarse, const RenderWs& ws, hipStream_t st) {
    constexpr int C = RENDER_C;
    if (p.warped) {
        if (int e = sk_warped_stratified(rays, p.u_strat, p.N, C, p.seed(), p.ray0(), p.near, p.far, p.gn, p.gf, ws.s_c, ws.z_c, nullptr, st))
            return hip_status(e, "warped stratified draw");
        const nerf_amd_samples sc = ray_samples(p, rays, C, ws.z_c, C);
        if (int e = launch_proposal_any(p.lflags, p.packed_prop, p.precision, sc, ws.density, st)) return hip_status(e, "proposal MLP");
        return hip_status(sk_warped_resample(ws.density, ws.s_c, rays + 3, 6, p.u_inv, p.N, C, K, 0, 0.01f, p.near, p.far, p.gn, p.gf, p.seed(), p.ray0(), z_out, s_out,
                                             nullptr, nullptr, st), "warped resample");
    }
    const float jitter = (p.far - p.near) / (float)p.n_fine;      // procedures.py:59
    nerf_amd_samples sc = ray_samples(p, rays, C, nullptr, C);
    sc.z_base = p.z_base; sc.u = p.u_strat; sc.z_jitter = jitter; sc.rng_seed = p.seed(); sc.rng_ray_offset = p.ray0();
    if (int e = launch_proposal_any(p.lflags, p.packed_prop, p.precision, sc, ws.density, st)) return hip_status(e, "proposal MLP");
    return hip_status(sk_resample(ws.density, nullptr, p.z_base, p.u_strat, jitter, rays + 3, 6, p.u_inv, p.N, C, K, 0, 0.01f, p.seed(), p.ray0(), z_out, nullptr, nullptr,
                                  z_coarse, st), "resample");
}
// the second round: the proposal network at the first round's P depths, then the n_fine + 1 fine depths from that histogram with columns
// [P, P + n_fine + 1) of each ray's inverse-CDF stream (the first round used [0, P))
int second_round(const RenderPlan& p, const float* rays, const RenderWs& ws, hipStream_t st) {
    const int P = p.prop_pnum, K = p.n_fine + 1;
    const nerf_amd_samples mid = ray_samples(p, rays, P, ws.z_mid, P);
    if (int e = launch_proposal_any(p.lflags, p.packed_prop, p.precision, mid, ws.density2, st)) return hip_status(e, "proposal MLP, second round");
    if (p.warped)
        return hip_status(sk_warped_resample_window(ws.density2, ws.s_mid, rays + 3, 6, p.N, P, K, P, 0.01f, p.near, p.far, p.gn, p.gf, p.seed(), p.ray0(), ws.z_fine,
                                                    nullptr, st), "warped resample, second round");
    return hip_status(sk_resample_window(ws.density2, ws.z_mid, rays + 3, 6, p.N, P, K, P, 0.01f, p.seed(), p.ray0(), ws.z_fine, st), "resample, second round");
}
// rows 8-9: drop the last depth, length2pts fused into the fine MLP (`dir_norm`: integrated PE, frustum s = [z_fine[s], z_fine[s+1]])
// (the empty-ray skip hands over its compact ray table and depth rows, n_rays of them: ws.rgbo then holds compact rows)
int fine_pass(const RenderPlan& p, const float* rays, const float* z_fine, int64_t n_rays, const float* dir_norm, const RenderWs& ws, hipStream_t st) {
    nerf_amd_samples sf = ray_samples(p, rays, p.n_fine, z_fine, p.n_fine + 1, n_rays);
    if (dir_norm) { sf.ipe = 1; sf.ipe_radius = p.camera->ipe_radius; sf.ipe_dir_norm = dir_norm; }
    return hip_status(launch_mip_any(p.lflags, p.packed_fine, p.precision, sf, ws.rgbo, st), "fine MLP");
}
// row 10.  Rows 9 and 10 are two launches: measured 2-3 % faster than the fused epilogue of nerf_amd_mip_forward_composite on MI355X
// (DESIGN.md section 3.3), and the composite kernel's HBM rate stays individually measurable.  Disparity spacing: composited with near = 0,
// far = 1 -- the kernel's depth is then the raw expected metric depth sum w z |d| -- and un-warped by one more launch.
// `rows` (the empty-ray skip; else NULL): ws.rgbo holds compact rows, ray n's at rows[n], none (zeros) where that is -1.
int composite_pass(const RenderPlan& p, const float* rays, const int32_t* rows, const RenderWs& ws, hipStream_t st) {
    const int flags = 1 | (p.white_bkg ? 2 : 0);
    const bool unwarp = p.warped && p.depth;
    const float near = p.warped ? 0.0f : p.near, far = p.warped ? 1.0f : p.far;
    float* depth = unwarp ? ws.depth_raw : p.depth;
    if (int e = rows ? sk_composite_rows(ws.rgbo, rows, ws.z_fine, p.n_fine + 1, rays + 3, 6, p.N, p.n_fine, flags, NERF_AMD_ACT_RELU, 0.0f, near, far, nullptr, nullptr,
                                         p.rgb, p.weights, depth, nullptr, st)
                     : sk_composite(ws.rgbo, ws.z_fine, p.n_fine + 1, rays + 3, 6, p.N, p.n_fine, flags, NERF_AMD_ACT_RELU, 0.0f, near, far, nullptr, nullptr, p.rgb,
                                    p.weights, depth, nullptr, st)) return hip_status(e, "composite");
    return unwarp ? hip_status(sk_warp_depths(ws.depth_raw, nullptr, p.N, 1, 1, p.near, p.far, p.gn, p.gf, p.depth, nullptr, st), "depth un-warp") : NERF_AMD_OK;
}
// nerf_amd_render's optional outputs, appended to the entry point's launches (nothing is launched when none is asked for): the stats
// kernel on the weights and the depth row (stride = row length) the fine pass composited [-> un-warp] [-> a copy of the depth row]
int extras_pass(const RenderPlan& p, const float* rays, const float* z_row, bool closed, const RenderExtrasWs& x, hipStream_t st) {
    const int S = p.fine_samples(), E = S + (closed ? 1 : 0);
    if (p.want_stats()) {
        float* dq = p.depth_q && p.n_quantiles ? (p.warped ? x.depth_q_raw : p.depth_q) : nullptr;
        if (int e = sk_ray_depth_stats(p.weights, z_row, E, closed, rays + 3, 6, p.N, S, 1, p.quantiles, p.n_quantiles, p.warped ? 0.0f : p.near,
                                       p.warped ? 1.0f : p.far, p.opacity, dq, st)) return hip_status(e, "depth quantiles and opacity");
        if (dq && p.warped)
            if (int e = sk_warp_depths(dq, nullptr, p.N, p.n_quantiles, 1, p.near, p.far, p.gn, p.gf, p.depth_q, nullptr, st)) return hip_status(e, "quantile un-warp");
    }
    if (p.fine_depths) return hip_status((int)hipMemcpyAsync(p.fine_depths, z_row, (size_t)p.N * E * 4, hipMemcpyDeviceToDevice, st), "fine depth copy");
    return NERF_AMD_OK;
}
// The empty-ray skip (include/nerf_amd.h), between the last resampling and the fine pass: flags and ordered compaction of the histogram
// (density, z) of C depths per ray, N' read back to the host -- the one synchronisation of a render call, which is why the mode cannot be
// captured --, then the alive rays' ray records and fine depth rows (z_rows, E floats each) gathered into the compact tables.
int skip_stage(const RenderPlan& p, const float* rays, const float* density, const float* z, int C, const float* z_rows, const RenderExtrasWs& x, hipStream_t st,
               int64_t* n_alive, const int32_t** rows) {
    int32_t* row_of_ray = p.row_of_ray ? p.row_of_ray : x.row_of_ray;
    if (int e = sk_ray_alive(density, z, C, rays + 3, 6, p.N, C, p.skip_dmin, row_of_ray, x.ray_of_row, x.count, x.alive_ws, st)) return hip_status(e, "empty-ray flags and compaction");
    int64_t count = -1;
    if (int e = (int)hipMemcpyAsync(&count, x.count, sizeof count, hipMemcpyDeviceToHost, st)) return hip_status(e, "alive-ray count read-back");
    if (int e = (int)hipStreamSynchronize(st)) return hip_status(e, "alive-ray count read-back");
    if (count < 0 || count > p.N) return fail(NERF_AMD_EHIP, "the alive-ray count read back from the device is outside 0..N");
    if (p.n_alive) *p.n_alive = count;
    *n_alive = count;
    *rows = row_of_ray;
    if (int e = sk_gather_rows(rays, 6, x.ray_of_row, count, 6, x.rays_c, st)) return hip_status(e, "ray gather");
    return hip_status(sk_gather_rows(z_rows, p.fine_row(), x.ray_of_row, count, p.fine_row(), x.z_rows_c, st), "depth row gather");
}
// refused before the first launch: a capturing stream (the skip reads a count on the host)
int check_skip_stream(const RenderPlan& p, hipStream_t st) {
    if (!p.skip()) return NERF_AMD_OK;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (int e = (int)hipStreamIsCapturing(st, &status)) return hip_status(e, "hipStreamIsCapturing");
    return status == hipStreamCaptureStatusNone ? NERF_AMD_OK
                                                : fail(NERF_AMD_EUNSUPPORTED, "the empty-ray skip reads the alive-ray count on the host: not on a capturing stream");
}
// the three MipNeRF entry points behind their own checks: shape, N == 0, inputs, then the launches in pipeline order
int render_mip(RenderPlan& p, void* workspace, hipStream_t st) {
    if (int e = check_plan_shape(p, NERF_AMD_PROP_W128 | NERF_AMD_FINE_W128, "unknown precision")) return e;
    if (p.N == 0) return NERF_AMD_OK;
    if (int e = check_plan_inputs(p, workspace)) return e;
    if (int e = check_skip_stream(p, st)) return e;
    const RenderWs ws = p.ws(workspace);
    const RenderExtrasWs x(p, workspace);
    const float *rays, *dir_norm;
    if (int e = provide_rays(p, ws, st, &rays)) return e;
    if (int e = provide_dir_norm(p, rays, ws, st, &dir_norm)) return e;       // (of the whole ray list: the skip compacts after it)
    const int P = p.prop_pnum;
    if (int e = coarse_pass(p, rays, P ? P : p.n_fine + 1, P ? ws.z_mid : ws.z_fine, P ? ws.s_mid : nullptr, x.z_coarse, ws, st)) return e;
    if (P)
        if (int e = second_round(p, rays, ws, st)) return e;
    const int32_t* rows = nullptr;                          // the skip: the histogram the fine depths were drawn from -> compact rays and depth rows
    const float *fine_rays = rays, *fine_z = ws.z_fine;
    int64_t n_fine_rays = p.N;
    if (p.skip()) {
        if (int e = skip_stage(p, rays, P ? ws.density2 : ws.density, P ? ws.z_mid : (p.warped ? ws.z_c : x.z_coarse), P ? P : RENDER_C, ws.z_fine, x, st, &n_fine_rays,
                               &rows)) return e;
        fine_rays = x.rays_c; fine_z = x.z_rows_c;
    }
    if (n_fine_rays)
        if (int e = fine_pass(p, fine_rays, fine_z, n_fine_rays, dir_norm, ws, st)) return e;
    if (x.weights) p.weights = x.weights;                   // (nerf_amd_render with stats and no weights output: composited into the appended part)
    if (int e = composite_pass(p, rays, rows, ws, st)) return e;
    return extras_pass(p, rays, ws.z_fine, true, x, st);
}
// the Ref-NeRF entry point, likewise: the checks, then the launches in pipeline order
int render_ref(RenderPlan& p, void* workspace, hipStream_t st) {
    if (bad_ref_flags(p.ref_flags)) return fail(NERF_AMD_EINVAL, "unknown precision or ref_flags");
    if (int e = check_plan_shape(p, NERF_AMD_PROP_W128, "unknown precision or ref_flags")) return e;
    if (p.N == 0) return NERF_AMD_OK;
    if (int e = check_plan_inputs(p, workspace)) return e;
    if ((p.normal_img != nullptr) != (p.cam_dir != nullptr)) return fail(NERF_AMD_EINVAL, "normal_img and cam_dir go together");
    if (int e = check_skip_stream(p, st)) return e;
    constexpr int C = RENDER_C;
    const int S_all = p.fine_samples();                     // (n_fine + 1) fine + 64 coarse depths, the last one dropped
    const RenderWs ws = p.ws(workspace);
    const float* rays;
    if (int e = provide_rays(p, ws, st, &rays)) return e;
    if (int e = coarse_pass(p, rays, p.n_fine + 1, ws.z_fine, nullptr, ws.z_coarse, ws, st)) return e;
    // row 8, Ref-NeRF branch (procedures.py:71-74): fine and coarse depths merged, the last one dropped
    if (int e = sk_merge_sorted(ws.z_fine, ws.z_coarse, p.N, p.n_fine + 1, C, ws.z_all, st)) return hip_status(e, "depth merge");
    const RenderExtrasWs x(p, workspace);
    const int32_t* rows = nullptr;                          // the skip: compact rays and merged depth rows, compact rgbo / normal rows
    const float *fine_rays = rays, *fine_z = ws.z_all;
    int64_t n_fine_rays = p.N;
    if (p.skip()) {
        if (int e = skip_stage(p, rays, ws.density, ws.z_coarse, C, ws.z_all, x, st, &n_fine_rays, &rows)) return e;
        fine_rays = x.rays_c; fine_z = x.z_rows_c;
    }
    const nerf_amd_samples sf = ray_samples(p, fine_rays, S_all, fine_z, S_all, n_fine_rays);   // row 13
    float* normals = p.normal_img ? ws.normals : nullptr;
    if (n_fine_rays)
        if (int e = mlp_launch_ref(p.packed_fine, p.precision, sf, ws.rgbo, normals, nullptr, p.ref_flags, st)) return hip_status(e, "Ref-NeRF MLP");
    if (x.weights) p.weights = x.weights;
    const int flags = 1 | (p.white_bkg ? 2 : 0);            // row 10 with sigma -> softplus(sigma + 0.5) (procedures.py:73)
    if (int e = rows ? sk_composite_rows(ws.rgbo, rows, ws.z_all, S_all, rays + 3, 6, p.N, S_all, flags, NERF_AMD_ACT_SOFTPLUS, 0.5f, p.near, p.far, normals, p.cam_dir, p.rgb,
                                         p.weights, p.depth, p.normal_img, st)
                     : sk_composite(ws.rgbo, ws.z_all, S_all, rays + 3, 6, p.N, S_all, flags, NERF_AMD_ACT_SOFTPLUS, 0.5f, p.near, p.far, normals, p.cam_dir, p.rgb, p.weights,
                                    p.depth, p.normal_img, st)) return hip_status(e, "composite");
    return extras_pass(p, rays, ws.z_all, false, x, st);
}
// the sizes nerf_amd_render_rays_rounds takes, for the entry point and its workspace query alike: NULL, or what is wrong
const char* rounds_shape_error(int64_t N, int n_fine, int prop_pnum, int spacing) {
    if (spacing != NERF_AMD_SPACING_LINEAR && spacing != NERF_AMD_SPACING_DISPARITY) return "unknown spacing (NERF_AMD_SPACING_LINEAR or NERF_AMD_SPACING_DISPARITY)";
    if (N < 0 || n_fine < 1 || n_fine > 1023) return "bad N or n_fine (1 <= n_fine <= 1023)";
    if (prop_pnum < 3 || prop_pnum > 256) return "bad prop_pnum (3 <= prop_pnum <= 256: the second round's histogram)";
    return nullptr;
}
// request -> plan, the one place a plan is filled: which pipeline (ref, prop_pnum, spacing) and what is refused before it starts
int plan_from_request(const nerf_amd_render_request* r, RenderPlan& p, bool sizing) {     // sizing: the workspace query, which needs no descriptor
    if (!r) return fail(NERF_AMD_EINVAL, "NULL argument: request");
    constexpr size_t first_layout = offsetof(nerf_amd_render_request, skip_min_optical_depth);     // everything up to fine_depths
    if (r->size < first_layout) return fail(NERF_AMD_EINVAL, "request->size is smaller than nerf_amd_render_request");
    const bool has_skip = r->size >= sizeof(nerf_amd_render_request);
    if (r->spacing != NERF_AMD_SPACING_LINEAR && r->spacing != NERF_AMD_SPACING_DISPARITY)
        return fail(NERF_AMD_EINVAL, "unknown spacing (NERF_AMD_SPACING_LINEAR or NERF_AMD_SPACING_DISPARITY)");
    const bool warped = r->spacing == NERF_AMD_SPACING_DISPARITY, rounds = !r->ref && r->prop_pnum != 0;
    if (r->ref && (warped || r->prop_pnum)) return fail(NERF_AMD_EUNSUPPORTED, "the Ref-NeRF pipeline has neither disparity spacing nor a second proposal round");
    if (rounds) {
        if (const char* bad_shape = rounds_shape_error(r->N, r->n_fine, r->prop_pnum, r->spacing)) return fail(NERF_AMD_EINVAL, bad_shape);
        if (r->u_strat || r->u_inv) return fail(NERF_AMD_EINVAL, "two proposal rounds draw their uniforms in the kernels: u_strat and u_inv must be NULL");
    }
    p = RenderPlan{r->packed_prop, r->packed_fine, r->precision, 0, r->rays, r->camera, r->ray_offset, warped ? nullptr : r->z_base, r->u_strat, r->u_inv, r->N, r->n_fine,
                   rounds ? r->prop_pnum : 0, warped, r->ref != 0, r->near, r->far, 0.0f, 0.0f, r->white_bkg, r->rgb, r->depth, r->weights};
    if (warped)
        if (int e = check_spacing(r->spacing, r->near, r->far, &p.gn, &p.gf)) return e;
    if (rounds && !sizing && r->N && !r->camera) return fail(NERF_AMD_EINVAL, "NULL argument: in-kernel uniforms need the descriptor (rng_seed, rng_ray_offset)");
    if (p.ref) { p.ref_flags = r->ref_flags; p.cam_dir = r->cam_dir; p.normal_img = r->normal_img; }
    if (int e = check_quantiles(r->quantiles, r->n_quantiles)) return e;
    p.opacity = r->opacity; p.depth_q = r->depth_q; p.fine_depths = r->fine_depths; p.n_quantiles = r->n_quantiles;
    for (int j = 0; j < r->n_quantiles; ++j) p.quantiles[j] = r->quantiles[j];
    if (has_skip) {
        if (r->skip_min_optical_depth != r->skip_min_optical_depth) return fail(NERF_AMD_EINVAL, "skip_min_optical_depth is NaN");
        if (r->skip_min_optical_depth > 0.0) { p.skip_dmin = r->skip_min_optical_depth; p.row_of_ray = r->row_of_ray; p.n_alive = r->n_alive; }
    }
    return NERF_AMD_OK;
}
// every render entry point ends here: nerf_amd_render directly, the four argument-list entry points with a request they fill themselves
int render_request(const nerf_amd_render_request* r, void* workspace, void* stream) {
    RenderPlan p{};
    if (int e = plan_from_request(r, p, false)) return e;
    if (p.skip() && p.N == 0 && p.n_alive) *p.n_alive = 0;  // (no ray, none alive: the pipelines return before their first stage)
    return p.ref ? render_ref(p, workspace, S(stream)) : render_mip(p, workspace, S(stream));
}
}  // namespace

size_t nerf_amd_render_workspace_bytes(int64_t N, int n_fine) { return render_ws_bytes(false, false, N, n_fine); }
int nerf_amd_render_rays(const void* packed_prop, const void* packed_mip, int precision, const float* rays, const nerf_amd_samples* camera,
                         int64_t ray_offset, const float* z_base, const float* u_strat, const float* u_inv, int64_t N, int n_fine, float near, float far,
                         int white_bkg, float* rgb, float* depth, float* weights, void* workspace, void* stream) {
    nerf_amd_render_request r{};
    r.size = sizeof r; r.packed_prop = packed_prop; r.packed_fine = packed_mip; r.precision = precision; r.rays = rays; r.camera = camera;
    r.ray_offset = ray_offset; r.z_base = z_base; r.u_strat = u_strat; r.u_inv = u_inv; r.N = N; r.n_fine = n_fine; r.spacing = NERF_AMD_SPACING_LINEAR;
    r.near = near; r.far = far; r.white_bkg = white_bkg; r.rgb = rgb; r.depth = depth; r.weights = weights;
    return render_request(&r, workspace, stream);
}

// ------------------------------------------------------------------------------------------------ disparity ray spacing
int nerf_amd_warp_depths(const float* in, const float* rays, int64_t N, int Sn, int inverse, int spacing, float near, float far, float* out, float* pts,
                         void* stream) {
    float gn, gf;
    if (int e = check_spacing(spacing, near, far, &gn, &gf)) return e;
    if (N < 0 || Sn < 1) return fail(NERF_AMD_EINVAL, "need N >= 0 and S >= 1");
    if (N && (!in || !out || (pts && !rays))) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (pts && inverse) return fail(NERF_AMD_EINVAL, "pts are positions o + z d: not with inverse");
    return hip_status(sk_warp_depths(in, rays, N, Sn, inverse ? 1 : 0, near, far, gn, gf, out, pts, S(stream)), "nerf_amd_warp_depths");
}

int nerf_amd_warped_stratified(const float* rays, const float* u, int64_t N, int C, uint64_t rng_seed, int64_t rng_ray_offset, int spacing, float near,
                               float far, float* s_c, float* z_c, float* pts, void* stream) {
    float gn, gf;
    if (int e = check_spacing(spacing, near, far, &gn, &gf)) return e;
    if (N < 0 || C < 3 || C > 256) return fail(NERF_AMD_EINVAL, "need N >= 0 and 3 <= C <= 256");
    if (!u && C > 64) return fail(NERF_AMD_EINVAL, "the stratified Philox stream has 64 slots per ray: pass u for C > 64");
    if (N && (!s_c || !z_c || (pts && !rays))) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_warped_stratified(rays, u, N, C, rng_seed, rng_ray_offset, near, far, gn, gf, s_c, z_c, pts, S(stream)), "nerf_amd_warped_stratified");
}

int nerf_amd_warped_resample(const float* density, const float* s_c, const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K,
                             int softplus_density, float blur_alpha, int spacing, float near, float far, uint64_t rng_seed, int64_t rng_ray_offset,
                             float* z_fine, float* s_fine, int64_t* below, float* w_prop, void* stream) {
    float gn, gf;
    if (int e = check_spacing(spacing, near, far, &gn, &gf)) return e;
    if (N < 0) return fail(NERF_AMD_EINVAL, "negative ray count");
    if (int e = check_warped_resample_shape(C, K)) return e;
    if (dirs_stride < 3) return fail(NERF_AMD_EINVAL, "dirs_stride < 3");
    if (N && (!density || !s_c || !dirs || !z_fine)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_warped_resample(density, s_c, dirs, dirs_stride, u_inv, N, C, K, softplus_density, blur_alpha, near, far, gn, gf, rng_seed,
                                         rng_ray_offset, z_fine, s_fine, below, w_prop, S(stream)), "nerf_amd_warped_resample");
}

size_t nerf_amd_render_warped_workspace_bytes(int64_t N, int n_fine) { return render_ws_bytes(true, false, N, n_fine); }
int nerf_amd_render_rays_warped(const void* packed_prop, const void* packed_mip, int precision, const float* rays, const nerf_amd_samples* camera,
                                int64_t ray_offset, const float* u_strat, const float* u_inv, int64_t N, int n_fine, int spacing, float near, float far,
                                int white_bkg, float* rgb, float* depth, float* weights, void* workspace, void* stream) {
    // (the request takes NERF_AMD_SPACING_LINEAR as the linear pipeline and words an unknown value differently: refused here, with check_spacing's text)
    if (spacing != NERF_AMD_SPACING_DISPARITY) return fail(NERF_AMD_EINVAL, "unknown spacing (the warped entry points take NERF_AMD_SPACING_DISPARITY only)");
    nerf_amd_render_request r{};
    r.size = sizeof r; r.packed_prop = packed_prop; r.packed_fine = packed_mip; r.precision = precision; r.rays = rays; r.camera = camera;
    r.ray_offset = ray_offset; r.u_strat = u_strat; r.u_inv = u_inv; r.N = N; r.n_fine = n_fine; r.spacing = spacing;
    r.near = near; r.far = far; r.white_bkg = white_bkg; r.rgb = rgb; r.depth = depth; r.weights = weights;
    return render_request(&r, workspace, stream);
}

// ------------------------------------------------------------------------------------------------ two proposal rounds
size_t nerf_amd_render_rounds_workspace_bytes(int64_t N, int n_fine, int prop_pnum, int spacing) {
    return rounds_shape_error(N, n_fine, prop_pnum, spacing) ? 0 : RenderWs(spacing == NERF_AMD_SPACING_DISPARITY, prop_pnum, false, nullptr, N, n_fine).bytes;
}
int nerf_amd_render_rays_rounds(const void* packed_prop, const void* packed_mip, int precision, const float* rays, const nerf_amd_samples* camera,
                                int64_t ray_offset, const float* z_base, int64_t N, int n_fine, int prop_pnum, int spacing, float near, float far, int white_bkg,
                                float* rgb, float* depth, float* weights, void* workspace, void* stream) {
    // (first and here: to the request prop_pnum == 0 means one round)
    if (const char* bad_shape = rounds_shape_error(N, n_fine, prop_pnum, spacing)) return fail(NERF_AMD_EINVAL, bad_shape);
    nerf_amd_render_request r{};
    r.size = sizeof r; r.packed_prop = packed_prop; r.packed_fine = packed_mip; r.precision = precision; r.rays = rays; r.camera = camera;
    r.ray_offset = ray_offset; r.z_base = z_base; r.N = N; r.n_fine = n_fine; r.prop_pnum = prop_pnum; r.spacing = spacing;
    r.near = near; r.far = far; r.white_bkg = white_bkg; r.rgb = rgb; r.depth = depth; r.weights = weights;
    return render_request(&r, workspace, stream);
}

size_t nerf_amd_render_ref_workspace_bytes(int64_t N, int n_fine) { return render_ws_bytes(false, true, N, n_fine); }
int nerf_amd_render_rays_ref(const void* packed_prop, const void* packed_ref, int precision, int ref_flags, const float* rays, const nerf_amd_samples* camera,
                             int64_t ray_offset, const float* z_base, const float* u_strat, const float* u_inv, int64_t N, int n_fine, float near, float far,
                             int white_bkg, const float* cam_dir, float* rgb, float* depth, float* normal_img, void* workspace, void* stream) {
    nerf_amd_render_request r{};
    r.size = sizeof r; r.packed_prop = packed_prop; r.packed_fine = packed_ref; r.precision = precision; r.ref = 1; r.ref_flags = ref_flags; r.rays = rays;
    r.camera = camera; r.ray_offset = ray_offset; r.z_base = z_base; r.u_strat = u_strat; r.u_inv = u_inv; r.N = N; r.n_fine = n_fine;
    r.spacing = NERF_AMD_SPACING_LINEAR; r.near = near; r.far = far; r.white_bkg = white_bkg; r.cam_dir = cam_dir; r.rgb = rgb; r.depth = depth;
    r.normal_img = normal_img;
    return render_request(&r, workspace, stream);
}

// ------------------------------------------------------------------------------------------------ one request for all four, with the optional outputs
size_t nerf_amd_render_request_workspace_bytes(const nerf_amd_render_request* request) {
    RenderPlan p{};
    if (plan_from_request(request, p, true) || p.N < 0 || p.n_fine < 1) return 0;
    return RenderExtrasWs(p, nullptr).bytes;
}
int nerf_amd_render(const nerf_amd_render_request* request, void* workspace, void* stream) {
    return render_request(request, workspace, stream);
}

size_t nerf_amd_ray_alive_workspace_bytes(int64_t N) { return (N < 0 || N > 0x7fffffff) ? 0 : sk_ray_alive_workspace_bytes(N); }
int nerf_amd_ray_alive(const float* density, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int C, double min_optical_depth,
                       int32_t* row_of_ray, int64_t* ray_of_row, int64_t* count_dev, void* workspace, void* stream) {
    if (N < 0 || N > 0x7fffffff) return fail(NERF_AMD_EINVAL, "need 0 <= N < 2^31 (rays are ranked in int32)");
    if (C < 2) return fail(NERF_AMD_EINVAL, "need C >= 2 depths per ray");
    if (z_stride < C) return fail(NERF_AMD_EINVAL, "z_stride is smaller than the depth row (C)");
    if (dirs_stride < 3) return fail(NERF_AMD_EINVAL, "dirs_stride < 3");
    if (min_optical_depth != min_optical_depth) return fail(NERF_AMD_EINVAL, "min_optical_depth is NaN");
    if (!count_dev) return fail(NERF_AMD_EINVAL, "NULL argument: count_dev");
    if (N && (!density || !z || !dirs || !row_of_ray || !ray_of_row || !workspace)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_ray_alive(density, z, z_stride, dirs, dirs_stride, N, C, min_optical_depth, row_of_ray, ray_of_row, count_dev, workspace, S(stream)),
                      "nerf_amd_ray_alive");
}
int nerf_amd_gather_rows(const float* src, int64_t src_stride, const int64_t* ray_of_row, int64_t n_rows, int cols, float* dst, void* stream) {
    if (n_rows < 0 || cols < 0 || src_stride < cols) return fail(NERF_AMD_EINVAL, "bad size or stride (n_rows >= 0, 0 <= cols <= src_stride)");
    if (n_rows * cols && (!src || !ray_of_row || !dst)) return fail(NERF_AMD_EINVAL, "NULL argument");
    return hip_status(sk_gather_rows(src, src_stride, ray_of_row, n_rows, cols, dst, S(stream)), "nerf_amd_gather_rows");
}

int nerf_amd_ray_depth_stats(const float* weights, const float* z, int z_stride, int closed, const float* dirs, int dirs_stride, int64_t N, int Sn, int mul_norm,
                             const float* quantiles, int n_quantiles, float near, float far, float* opacity, float* depth_q, void* stream) {
    if (N < 0 || Sn < 1) return fail(NERF_AMD_EINVAL, "need N >= 0 and S >= 1");
    if (int e = check_quantiles(quantiles, n_quantiles)) return e;
    if (z_stride < Sn + (closed ? 1 : 0)) return fail(NERF_AMD_EINVAL, "z_stride is smaller than the depth row (S + 1 depths of a closed row, S of an open one)");
    if (mul_norm && dirs_stride < 3) return fail(NERF_AMD_EINVAL, "dirs_stride < 3");
    if (N && (!weights || !z || (mul_norm && !dirs))) return fail(NERF_AMD_EINVAL, "NULL argument");
    if (N && n_quantiles && !depth_q) return fail(NERF_AMD_EINVAL, "NULL argument: depth_q (with n_quantiles > 0)");
    return hip_status(sk_ray_depth_stats(weights, z, z_stride, closed, dirs, dirs_stride, N, Sn, mul_norm, quantiles, n_quantiles, near, far, opacity, depth_q,
                                         S(stream)), "nerf_amd_ray_depth_stats");
}

size_t nerf_amd_gemm_workspace_bytes(int64_t M, int64_t N, int64_t P) {
    if (M <= 0 || N <= 0 || P <= 0) return 0;
    return gk_gemm_workspace_bytes(M, N, P);
}

int nerf_amd_gemm(int precision, int64_t M, int64_t N, int64_t P, const float* A, int64_t a_si, int64_t a_sp, const float* B, int64_t b_sp, int64_t b_sj,
                  float* C, int64_t ldc, const float* bias, int act, const float* mask, int64_t ldm, void* workspace, void* stream) {
    if (precision != NERF_AMD_F32 && precision != NERF_AMD_BF16) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: precision must be NERF_AMD_F32 or NERF_AMD_BF16");
    if (M < 0 || N < 0 || P < 0 || N > 65535LL * 128) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: bad size");
    if (M == 0 || N == 0) return 0;
    if (!C || (P && (!A || !B))) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: NULL argument");
    if ((a_si != 1 && a_sp != 1) || (b_sp != 1 && b_sj != 1)) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: one stride of each operand must be 1");
    if (ldc < N || (mask && ldm < N)) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: row stride smaller than N");
    if (act < 0 || act > 2) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: act must be 0 (none), 1 (ReLU) or 2 (sigmoid)");
    if (gk_gemm_workspace_bytes(M, N, P) && !workspace) return fail(NERF_AMD_EINVAL, "nerf_amd_gemm: this shape needs nerf_amd_gemm_workspace_bytes of workspace");
    return hip_status(gk_gemm(precision == NERF_AMD_BF16, M, N, P, A, a_si, a_sp, B, b_sp, b_sj, C, ldc, bias, act, mask, ldm, workspace, S(stream)), "nerf_amd_gemm");
}

int nerf_amd_sigmoid_backward(const float* g, int64_t g_stride, const float* y, int64_t y_stride, int64_t M, int cols, float* out, int64_t out_stride,
                              void* stream) {
    if (M < 0 || cols < 0) return fail(NERF_AMD_EINVAL, "nerf_amd_sigmoid_backward: bad size");
    if (M * cols && (!g || !y || !out)) return fail(NERF_AMD_EINVAL, "nerf_amd_sigmoid_backward: NULL argument");
    if (g_stride < cols || y_stride < cols || out_stride < cols) return fail(NERF_AMD_EINVAL, "nerf_amd_sigmoid_backward: row stride smaller than cols");
    return hip_status(gk_sigmoid_backward(g, g_stride, y, y_stride, M, cols, out, out_stride, S(stream)), "nerf_amd_sigmoid_backward");
}

// ---- generic-shape Ref-NeRF: the element-wise stages between its layer products (generic_ref_kernels.hip) ----
int nerf_amd_ref_dir_inputs(const float* heads, int64_t heads_stride, const float* dirs, int64_t dirs_stride, int64_t M, int ide_level, const float* ide_table,
                            float* out, int64_t out_stride, float* normal, void* stream) {
    if (M < 0 || ide_level < 1 || ide_level > 5) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs: bad size / ide_level (1..5)");
    if (M && (!heads || !dirs || !ide_table || !out || !normal)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs: NULL argument");
    const int T = (1 << ide_level) - 1 + ide_level;
    if (heads_stride < 11 || dirs_stride < 3 || out_stride < 2 * T + 1) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs: row stride too small");
    return hip_status(gr_dir_inputs(heads, heads_stride, dirs, dirs_stride, M, ide_level, ide_table, out, out_stride, normal, S(stream)), "nerf_amd_ref_dir_inputs");
}

int nerf_amd_ref_dir_inputs_backward(const float* heads, int64_t heads_stride, const float* dirs, int64_t dirs_stride, int64_t M, int ide_level,
                                     const float* ide_table, const float* d_out, int64_t d_out_stride, const float* g_normal, int64_t g_normal_stride,
                                     float* d_heads, int64_t d_heads_stride, void* stream) {
    if (M < 0 || ide_level < 1 || ide_level > 5) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs_backward: bad size / ide_level (1..5)");
    if (M && (!heads || !dirs || !ide_table || !d_out || !g_normal || !d_heads)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs_backward: NULL argument");
    const int T = (1 << ide_level) - 1 + ide_level;
    if (heads_stride < 11 || dirs_stride < 3 || d_out_stride < 2 * T + 1 || g_normal_stride < 3 || d_heads_stride < 11)
        return fail(NERF_AMD_EINVAL, "nerf_amd_ref_dir_inputs_backward: row stride too small");
    return hip_status(gr_dir_inputs_backward(heads, heads_stride, dirs, dirs_stride, M, ide_level, ide_table, d_out, d_out_stride, g_normal, g_normal_stride, d_heads,
                                             d_heads_stride, S(stream)), "nerf_amd_ref_dir_inputs_backward");
}

int nerf_amd_ref_combine(const float* heads, int64_t heads_stride, const float* spec, int64_t spec_stride, int64_t M, int ref_flags, float* rgbo, void* stream) {
    if (M < 0 || bad_ref_flags(ref_flags)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine: bad size / ref_flags");
    if (M && (!heads || !spec || !rgbo)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine: NULL argument");
    if (heads_stride < 11 || spec_stride < 3) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine: row stride too small");
    return hip_status(gr_combine(heads, heads_stride, spec, spec_stride, M, (ref_flags & NERF_AMD_REF_SRGB) ? 1 : 0, rgbo, S(stream)), "nerf_amd_ref_combine");
}

int nerf_amd_ref_combine_backward(const float* g_rgbo, int64_t g_stride, const float* heads, int64_t heads_stride, const float* spec, int64_t spec_stride, int64_t M,
                                  int ref_flags, float* d_spec, int64_t d_spec_stride, float* d_heads, int64_t d_heads_stride, void* stream) {
    if (M < 0 || bad_ref_flags(ref_flags)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine_backward: bad size / ref_flags");
    if (M && (!g_rgbo || !heads || !spec || !d_spec || !d_heads)) return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine_backward: NULL argument");
    if (g_stride < 4 || heads_stride < 11 || spec_stride < 3 || d_spec_stride < 3 || d_heads_stride < 11)
        return fail(NERF_AMD_EINVAL, "nerf_amd_ref_combine_backward: row stride too small");
    return hip_status(gr_combine_backward(g_rgbo, g_stride, heads, heads_stride, spec, spec_stride, M, (ref_flags & NERF_AMD_REF_SRGB) ? 1 : 0, d_spec, d_spec_stride,
                                          d_heads, d_heads_stride, S(stream)), "nerf_amd_ref_combine_backward");
}

int nerf_amd_positional_encoding_backward(const float* d_enc, int64_t d_enc_stride, const float* x, int64_t x_stride, int64_t M, int L, int cat_origin, float* d_x,
                                          void* stream) {
    if (M < 0 || L < 0) return fail(NERF_AMD_EINVAL, "nerf_amd_positional_encoding_backward: bad size");
    if (M && (!d_enc || !x || !d_x)) return fail(NERF_AMD_EINVAL, "nerf_amd_positional_encoding_backward: NULL argument");
    if (d_enc_stride < 6 * L + (cat_origin ? 3 : 0) || x_stride < 3) return fail(NERF_AMD_EINVAL, "nerf_amd_positional_encoding_backward: row stride too small");
    return hip_status(gr_pe_backward(d_enc, d_enc_stride, x, x_stride, M, L, cat_origin ? 1 : 0, d_x, S(stream)), "nerf_amd_positional_encoding_backward");
}

int nerf_amd_contract_positions(const float* x, int64_t x_stride, int64_t M, const float* g, int64_t g_stride, float* out, void* stream) {
    if (M < 0 || x_stride < 3 || (g && g_stride < 3)) return fail(NERF_AMD_EINVAL, "nerf_amd_contract_positions: bad size or stride");
    if (M && (!x || !out)) return fail(NERF_AMD_EINVAL, "nerf_amd_contract_positions: NULL argument");
    return hip_status(gr_contract(x, x_stride, M, g, g_stride, out, S(stream)), "nerf_amd_contract_positions");
}

int nerf_amd_add_rows(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, int64_t M, int cols, void* stream) {
    if (M < 0 || cols < 0) return fail(NERF_AMD_EINVAL, "nerf_amd_add_rows: bad size");
    if (M * cols && (!dst || !src)) return fail(NERF_AMD_EINVAL, "nerf_amd_add_rows: NULL argument");
    if (dst_stride < cols || src_stride < cols) return fail(NERF_AMD_EINVAL, "nerf_amd_add_rows: row stride smaller than cols");
    return hip_status(gr_add_rows(dst, dst_stride, src, src_stride, M, cols, S(stream)), "nerf_amd_add_rows");
}

int nerf_amd_rows_gemm(int64_t M, int64_t N, int64_t K, const void* X, int64_t ldx, const void* W, int64_t ldw, int64_t n_pad, const float* bias, int act, void* C,
                       int64_t ldc, int out_bf16, void* stream) {
    if (M < 0 || N < 0 || K < 1 || N > 65535LL * 256) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: bad size");
    if (M == 0 || N == 0) return 0;
    if (!X || !W || !bias || !C) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: NULL argument");
    if (act < 0 || act > 2) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: act must be 0 (none), 1 (ReLU) or 2 (sigmoid)");
    if ((ldx & 7) || ldx < (K + 7) / 8 * 8 || (reinterpret_cast<uintptr_t>(X) & 15u))
        return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: X must be 16-byte aligned bf16 rows with a stride that is a multiple of 8 elements >= roundup(K, 8)");
    if ((ldw & 63) || ldw < K || (n_pad & 255) || n_pad < N || (reinterpret_cast<uintptr_t>(W) & 15u) || (reinterpret_cast<uintptr_t>(bias) & 15u))
        return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: W must be packed (n_pad % 256 == 0 rows >= N, ldw % 64 == 0 >= K, 16-byte aligned), bias 16-byte aligned");
    if (ldc < N) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: row stride of C smaller than N");
    if (out_bf16 && ((N & 3) || (ldc & 3) || (reinterpret_cast<uintptr_t>(C) & 7u)))
        return fail(NERF_AMD_EINVAL, "nerf_amd_rows_gemm: bf16 output needs N % 4 == 0, ldc % 4 == 0 and an 8-byte aligned C");
    return hip_status(rg_rows_gemm(M, N, K, X, ldx, W, ldw, n_pad, bias, act, C, ldc, out_bf16, S(stream)), "nerf_amd_rows_gemm");
}

int nerf_amd_rows_to_bf16(const float* src, int64_t rows_src, int64_t src_stride, int64_t rows, int cols, int fill, void* dst, int64_t dst_stride, void* stream) {
    if (rows < 0 || rows_src < 0 || rows_src > rows || cols < 0 || fill < cols) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_to_bf16: bad size");
    if (rows * fill == 0) return 0;
    if (!dst || (rows_src * cols && !src)) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_to_bf16: NULL argument");
    if (src_stride < cols || dst_stride < fill) return fail(NERF_AMD_EINVAL, "nerf_amd_rows_to_bf16: row stride smaller than the columns written");
    return hip_status(rg_rows_to_bf16(src, rows_src, src_stride, rows, cols, fill, dst, dst_stride, S(stream)), "nerf_amd_rows_to_bf16");
}

static int check_image_metrics_shape(int64_t V, int C, int H, int W) {
    if (V <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(NERF_AMD_EINVAL, "nerf_amd_image_metrics: V, C, H, W must be positive");
    if (H < 11 || W < 11) return fail(NERF_AMD_EINVAL, "nerf_amd_image_metrics: H and W must be at least 11 (the window; valid positions only)");
    // (factor by factor: none of the products can overflow)
    if (V > 0x7fffffffLL / C || im_workgroups(1, 1, H, W) > 0x7fffffffLL / (V * C)) return fail(NERF_AMD_EINVAL, "nerf_amd_image_metrics: too many segments (V * C * segments must stay below 2^31)");
    return NERF_AMD_OK;
}
size_t nerf_amd_image_metrics_workspace_bytes(int64_t V, int C, int H, int W) {
    if (check_image_metrics_shape(V, C, H, W)) return 0;
    return (size_t)im_workgroups(V, C, H, W) * 2 * sizeof(double);
}
int nerf_amd_image_metrics(const float* pred, const float* target, int64_t V, int C, int H, int W, double* mse_out, double* ssim_out, float* ssim_map, void* workspace,
                           void* stream) {
    if (int e = check_image_metrics_shape(V, C, H, W)) return e;
    if (!pred || !target || !mse_out || !ssim_out || !workspace) return fail(NERF_AMD_EINVAL, "nerf_amd_image_metrics: NULL argument (only ssim_map is optional)");
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return fail(NERF_AMD_EINVAL, "nerf_amd_image_metrics: the workspace must be 8-byte aligned");
    return hip_status(im_image_metrics(pred, target, V, C, H, W, mse_out, ssim_out, ssim_map, workspace, S(stream)), "nerf_amd_image_metrics");
}

static int check_mesh_shape(const char* name, int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(NERF_AMD_EINVAL, "%s: every dimension of the lattice must be at least 2", name);
    if ((int64_t)nx * ny > 0x7fffffffLL / nz) return fail(NERF_AMD_EINVAL, "%s: nx * ny * nz must stay below 2^31 (points are ranked in int32)", name);
    return NERF_AMD_OK;
}
static bool finite_f(float x) { return x - x == 0.0f; }
size_t nerf_amd_mesh_workspace_bytes(int nx, int ny, int nz) { return check_mesh_shape("nerf_amd_mesh_workspace_bytes", nx, ny, nz) ? 0 : mesh_workspace_bytes(nx, ny, nz); }
int nerf_amd_mesh_count(const float* field, int nx, int ny, int nz, float iso, int64_t* counts_dev, void* workspace, void* stream) {
    if (int e = check_mesh_shape("nerf_amd_mesh_count", nx, ny, nz)) return e;
    if (!finite_f(iso)) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_count: iso must be finite");
    if (!field || !counts_dev || !workspace) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_count: NULL argument");
    return hip_status(mesh_count(field, nx, ny, nz, iso, counts_dev, workspace, S(stream)), "nerf_amd_mesh_count");
}
int nerf_amd_mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin_host, const float* spacing_host, void* workspace,
                       int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces, void* stream) {
    if (int e = check_mesh_shape("nerf_amd_mesh_emit", nx, ny, nz)) return e;
    if (!finite_f(iso)) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: iso must be finite");
    if (!field || !origin_host || !spacing_host || !workspace) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: NULL argument");
    for (int c = 0; c < 3; ++c) {
        if (!finite_f(origin_host[c])) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: origin must be finite");
        if (!(spacing_host[c] > 0.0f) || !finite_f(spacing_host[c])) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: spacing must be positive and finite");
    }
    if (vertex_capacity < 0 || face_capacity < 0) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: negative capacity");
    if (vertex_capacity > 0x7fffffffLL || face_capacity > 0x7fffffffLL / 3)
        return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: the vertex count and three times the face count must stay below 2^31 (indices are int32)");
    if ((vertex_capacity && !vertices) || (face_capacity && !faces)) return fail(NERF_AMD_EINVAL, "nerf_amd_mesh_emit: NULL output with a non-zero capacity");
    return hip_status(mesh_emit(field, nx, ny, nz, iso, origin_host, spacing_host, workspace, vertex_capacity, face_capacity, vertices, normals, faces, S(stream)),
                      "nerf_amd_mesh_emit");
}

}  // extern "C"
