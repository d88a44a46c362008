// Every host function that one translation unit of libnerf_amd.so defines and another calls, declared ONCE.  The definitions are written qualified
// (int nk::sk_resample(...) {): one that drifts from its declaration here is a compile error in its own unit, not an unresolved symbol at load time.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/nerf_amd.h"

namespace nk {
// ---- mlp_kernels.hip
int mlp_launch_proposal(const void* packed, int precision, const nerf_amd_samples& s, float* density, hipStream_t st);
int mlp_launch_mip(const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, hipStream_t st);
int mlp_launch_dir_table(const float* rays, int64_t N, void* table, hipStream_t st);
int mlp_launch_mip128(const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, hipStream_t st);
int mlp_launch_mip_composite(const void* packed, int precision, const nerf_amd_samples& s, float* rgb, float* depth, float* weights, int white_bkg, float near, float far, hipStream_t st);
int mlp_launch_proposal128(const void* packed, int precision, const nerf_amd_samples& s, float* density, hipStream_t st);
int64_t mlp_train_n_sub(int precision, int64_t M);
size_t mlp_train_layer_stride(int precision, int64_t M);
size_t mlp_train_mask_stride(int precision, int64_t M);
int mlp_launch_proposal_train(const void* packed, int precision, const nerf_amd_samples& s, float* density, void* dump, hipStream_t st);
int mlp_launch_mip_train(const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, void* dump, hipStream_t st);
int mlp_launch_ref(const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, float* normal, const float* bn_noise, int flags, hipStream_t st);
int mlp_launch_ref_train(const void* packed, int precision, const nerf_amd_samples& s, float* rgbo, float* normal, const float* bn_noise, void* dump, float* aux, int flags, hipStream_t st,
                         unsigned long long seed, const unsigned long long* seed_dev, float noise_std);
// ---- bwd_kernels.hip
int bwd_launch_dir_chain(int precision, const char* stream, int64_t M, const char* masks, size_t ms, char* dlt, size_t ls, float* rows, hipStream_t st);
int bwd_launch_chain(int which, int precision, const void* blob, int start_frag, int64_t M, const void* act, void* dlt, float* rows, hipStream_t st);
int bwd_launch_prop_chain(const void* packed_bwd, int precision, const float* g_density, int64_t M, const void* act_dump, void* delta_dump, hipStream_t st);
int bwd_launch_mip_chain(const void* packed_bwd, int precision, const float* g_rgbo, const float* rgbo, int64_t M, const void* act_dump, void* delta_dump, hipStream_t st);
size_t bwd_wgrad_workspace_bytes(int net, int precision, int64_t M);
int bwd_prop_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, float* const* d_w, float* const* d_b, void* workspace, hipStream_t st);
int bwd_mip_weight_grads(int precision, int64_t M, const void* act_dump, const void* delta_dump, const float* const* w, const float* const* b, float* const* d_w, float* const* d_b,
                         void* workspace, hipStream_t st);
size_t bwd_density_grad_workspace_bytes(int precision, int64_t M);
int bwd_density_grad(int net, const void* blob, int precision, int64_t M, const void* act, const float* x, int x_stride, const float* scale, int scale_stride, float* out, void* workspace,
                     hipStream_t st, int contract);
size_t bwd_ref_workspace_bytes(int precision, int64_t M);
int bwd_ref_backward(const void* blob, int precision, int64_t M, const void* act, const float* aux, const float* dirs, int dir_stride, const float* g_out, int g_stride,
                     const float* ide_table, float* const* d_w, float* const* d_b, void* workspace, int flags, hipStream_t st);
int bwd_launch_adam(float* const* p, const float* const* g, float* const* m, float* const* v, const long long* n, int count, float* step, double lr, const double* lr_dev, double beta1,
                    double beta2, double eps, float grad_scale, hipStream_t st);
// ---- pack_kernels.hip
int pack_proposal(int precision, const float* const* w, const float* const* b, void* packed, hipStream_t st);
int pack_proposal128(int precision, const float* const* w, const float* const* b, void* packed, hipStream_t st);
int pack_mip(int precision, const float* const* w, const float* const* b, void* packed, hipStream_t st);
int pack_mip128(int precision, const float* const* w, const float* const* b, void* packed, hipStream_t st);
int pack_ref(int precision, const float* const* w, const float* const* b, void* packed, hipStream_t st);
int pack_proposal_bwd(int precision, const float* const* w, void* packed, hipStream_t st);
int pack_mip_bwd(int precision, const float* const* w, void* packed, hipStream_t st);
int pack_ref_bwd(int precision, const float* const* w, void* packed, hipStream_t st);
int pack_mfma_stream(int iters, int workgroups, int mode, float* sink, hipStream_t st);
// ---- sample_kernels.hip
// dynamic LDS bytes of the launch that a shape leads to (the C-ABI's shape checks)
size_t sk_inverse_sample_lds_bytes(int C, int K);
size_t sk_resample_lds_bytes(int C, int K);
size_t sk_warped_resample_lds_bytes(int C, int K);
size_t sk_resample_window_lds_bytes(int C, int K, int warped);
size_t sk_get_bounds_lds_bytes(int C);
size_t sk_get_bounds_backward_lds_bytes(int K);
size_t sk_merge_sorted_lds_bytes(int K, int C, int order);
int sk_positional_encoding(const float* x, int64_t M, int L, float* out, hipStream_t st);
// contract: 0 | 1 (the frustum mean) | NERF_AMD_CONTRACT_GAUSSIAN (mean and covariance) -- nerf_amd_ipe_feature, _contracted, _gaussian
int sk_ipe_feature(const float* z, const float* rays, int64_t N, int Sn, int L, float r2, const float* dir_norm, float* feat, float* mu, float* mu_t, int contract, hipStream_t st);
int sk_cone_parameters(const float* z, int64_t N, int Sn, float r2, float* mu_t, float* var_t, float* var_r, hipStream_t st);
int sk_dirs_norm(const float* rays, int64_t N, float* out, hipStream_t st);
int sk_dirs_norm_scratch(const float* rays, int64_t N, float* out, void* partials, hipStream_t st);
int sk_train_sampler(const float* rgbs, const int64_t* coords, int64_t P, const float* pose, const float* pose_dev, float fx, float fy, float near, float far, int64_t N, int C,
                     uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, hipStream_t st);
int sk_scene_sampler(const float* images, const float* poses, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1, int y0, int y1, float fx, float fy, float near,
                     float far, int64_t N, int C, uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index, hipStream_t st);
int sk_scene_sampler_camera(const float* images, const float* poses, const float* cameras, int64_t V, int H, int W, const int64_t* view_ids, int64_t K, int x0, int x1, int y0, int y1,
                            float near, float far, int64_t N, int C, uint64_t seed, const uint64_t* seed_dev, float* pts, float* lengths, float* rgb, float* rays, int64_t* index,
                            hipStream_t st);
int sk_generate_rays_camera(const float* pose, int H, int W, const float* camera, int64_t first, int64_t count, float* rays, hipStream_t st);
int sk_philox_normal(float* out, int64_t M, uint64_t seed, const uint64_t* seed_dev, float std, int64_t sample_offset, hipStream_t st);
int sk_philox_uniforms(float* out, int64_t N, int K, uint64_t seed, const uint64_t* seed_dev, int64_t ray_offset, int strat, hipStream_t st);
int sk_advance_seed(uint64_t* seed_dev, hipStream_t st);
int sk_generate_rays(const float* pose, int H, int W, float fx, float fy, int64_t first, int64_t count, float* rays, hipStream_t st);
int sk_pixel_rays(const float* pose, float fx, float fy, const int64_t* coords, int64_t N, float* rays, hipStream_t st);
int sk_stratified_points(const float* rays, const float* z_base, const float* u, float jitter, int64_t N, int S, float* z_out, float* pts, hipStream_t st);
int sk_length2pts(const float* rays, const float* z, int64_t N, int S, float* out, hipStream_t st);
int sk_sigma_to_weights(const float* sigma, const float* z, const float* dirs, int64_t N, int S, int act, float* w, hipStream_t st);
int sk_max_blur(const float* w, int64_t N, int S, float alpha, float* out, hipStream_t st);
int sk_inverse_sample(const float* w, const float* z, const float* u, int64_t N, int C, int K, int sort, int mode, float* z_out, int64_t* below, int64_t* above, hipStream_t st);
int sk_resample(const float* density, const float* z, const float* z_base, const float* u_strat, float z_jitter, const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C,
                int K, int softplus, float alpha, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, int64_t* below, float* w_prop, float* z_coarse, hipStream_t st);
int sk_warp_depths(const float* in, const float* rays, int64_t N, int S, int inverse, float near, float far, float gn, float gf, float* out, float* pts, hipStream_t st);
int sk_warped_stratified(const float* rays, const float* u, int64_t N, int C, uint64_t seed, int64_t ray_offset, float near, float far, float gn, float gf, float* s_out, float* z_out,
                         float* pts, hipStream_t st);
int sk_warped_resample(const float* density, const float* s_c, const float* dirs, int dirs_stride, const float* u_inv, int64_t N, int C, int K, int softplus, float alpha, float near,
                       float far, float gn, float gf, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, float* s_fine, int64_t* below, float* w_prop, hipStream_t st);
int sk_resample_window(const float* density, const float* z, const float* dirs, int dirs_stride, int64_t N, int C, int K, int u_col0, float alpha, uint64_t rng_seed,
                       int64_t rng_ray_offset, float* z_fine, hipStream_t st);
int sk_warped_resample_window(const float* density, const float* s_c, const float* dirs, int dirs_stride, int64_t N, int C, int K, int u_col0, float alpha, float near,
                              float far, float gn, float gf, uint64_t rng_seed, int64_t rng_ray_offset, float* z_fine, float* s_fine, hipStream_t st);
int sk_composite(const float* rgbo, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S, int flags, int act, float sigma_shift, float near, float far,
                 const float* normal, const float* cam_dir, float* rgb, float* weights, float* depth, float* normal_img, hipStream_t st);
// the same on COMPACT rgbo / normal rows: ray n reads row row_of_ray[n], an all-zero row where that is -1 (the empty-ray skip)
int sk_composite_rows(const float* rgbo, const int32_t* row_of_ray, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S, int flags, int act,
                      float sigma_shift, float near, float far, const float* normal, const float* cam_dir, float* rgb, float* weights, float* depth, float* normal_img, hipStream_t st);
// the empty-ray skip (nerf_amd_ray_alive / nerf_amd_gather_rows): N < 2^31; workspace of sk_ray_alive_workspace_bytes(N) bytes
size_t sk_ray_alive_workspace_bytes(int64_t N);
int sk_ray_alive(const float* density, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int C, double d_min, int32_t* row_of_ray, int64_t* ray_of_row,
                 int64_t* count_dev, void* workspace, hipStream_t st);
int sk_gather_rows(const float* src, int64_t src_stride, const int64_t* ray_of_row, int64_t n_rows, int cols, float* dst, hipStream_t st);
// quantiles: host, n_quantiles <= NERF_AMD_DEPTH_QUANTILES_MAX values in (0, 1), passed to the kernel by value (validated by the caller)
int sk_ray_depth_stats(const float* w, const float* z, int z_stride, int closed, const float* dirs, int dirs_stride, int64_t N, int S, int mul_norm,
                       const float* quantiles, int n_quantiles, float near, float far, float* opacity, float* depth_q, hipStream_t st);
int sk_get_bounds(const float* w, const int64_t* below, int64_t N, int C, int K, float* bounds, hipStream_t st);
int sk_weights_backward(const float* sigma, int sigma_stride, int sigma_off, const float* z, int z_stride, const float* dirs, int dirs_stride, int64_t N, int S, int mul_norm, int act,
                        float sigma_shift, const float* rgbo, const float* d_rgb, const float* d_weights, const float* d_depth, int white_bkg, float near, float far, float* d_sigma,
                        int d_sigma_stride, int d_sigma_off, float* d_rgbo, hipStream_t st);
int sk_max_blur_backward(const float* w, const float* g, int64_t N, int S, float* dw, hipStream_t st);
int sk_get_bounds_backward(const int64_t* below, const float* g, int64_t N, int C, int K, float* dw, hipStream_t st);
int sk_frag_to_rows(const void* frag, int elem_bytes, int64_t n_sub, int n_kg, int64_t M, void* out, hipStream_t st);
int sk_relu_mask(void* delta, const void* act, int elem_bytes, int64_t n, hipStream_t st);
int sk_relu_mask_bias(void* delta, const void* act, int elem_bytes, int64_t rows, int cols, float* col_sum, hipStream_t st);
int sk_merge_sorted(const float* a, const float* b, int64_t N, int K, int C, float* out, hipStream_t st);
int sk_merge_sorted_order(const float* a, const float* b, const int64_t* f_inds, int64_t N, int K, int C, float* out, int64_t* order, int64_t* all_inds, hipStream_t st);
int sk_coarse_grad_select(const float* grads, const int64_t* sort_inds, int64_t N, int T, int D, int c_pnum, float* out, hipStream_t st);
int sk_weighted_dot_loss(const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* out, float* workspace, hipStream_t st);
int sk_weighted_dot_loss_backward(const float* g, const float* w, const float* a, const float* b, int64_t M, int mode, float scale, float* d_w, float* d_a, float* d_b, hipStream_t st);
int sk_distortion_loss(const float* w, const float* t, int64_t N, int S, int mode, float scale, float* out, float* workspace, hipStream_t st);
int sk_distortion_loss_backward(const float* w, const float* t, int64_t N, int S, int mode, float scale, const float* g, float* d_w, float* d_t, hipStream_t st);
int sk_interlevel_loss(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale, float* out, float* bounds_out,
                       float* workspace, hipStream_t st);
int sk_interlevel_loss_backward(const float* w, const float* t, const float* w_prop, const float* t_prop, int64_t N, int M, int K, int Kp, float scale, const float* g, float* d_w_prop,
                                hipStream_t st);
int sk_encode_rows(const float* x, int x_stride, int64_t M, int L, int normalize, int elem_bytes, void* out, hipStream_t st);
int sk_frag_rows_mask_blocks();
int sk_frag_rows_mask(const void* frag, int elem_bytes, int64_t n_sub, int n_kg, int64_t M, void* act_out, void* delta, float* col_sum, hipStream_t st);
// ---- generic_kernels.hip
size_t gk_gemm_workspace_bytes(int64_t M, int64_t N, int64_t P);
int gk_gemm(int bf16, int64_t M, int64_t N, int64_t P, const float* A, int64_t a_si, int64_t a_sp, const float* B, int64_t b_sp, int64_t b_sj, float* C, int64_t ldc, const float* bias,
            int act, const float* mask, int64_t ldm, void* workspace, hipStream_t st);
int gk_sigmoid_backward(const float* g, int64_t gs, const float* y, int64_t ys, int64_t M, int cols, float* out, int64_t os, hipStream_t st);
// ---- generic_ref_kernels.hip
int gr_dir_inputs(const float* heads, int64_t ldh, const float* dirs, int64_t ds, int64_t M, int deg, const float* mat, float* out, int64_t ldo, float* normal, hipStream_t st);
int gr_dir_inputs_backward(const float* heads, int64_t ldh, const float* dirs, int64_t ds, int64_t M, int deg, const float* mat, const float* d_in, int64_t ldi, const float* g_normal,
                           int64_t ldg, float* d_heads, int64_t ldd, hipStream_t st);
int gr_combine(const float* heads, int64_t ldh, const float* spec, int64_t lds_, int64_t M, int srgb, float* rgbo, hipStream_t st);
int gr_combine_backward(const float* g, int64_t ldg, const float* heads, int64_t ldh, const float* spec, int64_t lds_, int64_t M, int srgb, float* d_spec, int64_t ldsp, float* d_heads,
                        int64_t ldd, hipStream_t st);
int gr_pe_backward(const float* d_enc, int64_t ldd, const float* x, int64_t ldx, int64_t M, int L, int cat_origin, float* d_x, hipStream_t st);
int gr_contract(const float* x, int64_t ldx, int64_t M, const float* g, int64_t ldg, float* out, hipStream_t st);
int gr_add_rows(float* dst, int64_t ldd, const float* src, int64_t lds_, int64_t M, int cols, hipStream_t st);
// ---- rows_gemm_kernels.hip
int rg_rows_gemm(int64_t M, int64_t N, int64_t K, const void* X, int64_t ldx, const void* W, int64_t ldw, int64_t n_pad, const float* bias, int act, void* C, int64_t ldc, int out_bf16,
                 hipStream_t st);
int rg_rows_to_bf16(const float* src, int64_t rows_src, int64_t lds, int64_t rows, int cols, int fill, void* dst, int64_t ldd, hipStream_t st);
// ---- image_metrics_kernels.hip
// workgroups (= fp64 pairs of workspace) of a call; H, W >= 11
int64_t im_workgroups(int64_t V, int C, int H, int W);
void im_window(float* g11);
int im_image_metrics(const float* pred, const float* target, int64_t V, int C, int H, int W, double* mse_out, double* ssim_out, float* ssim_map, void* workspace,
                     hipStream_t st);
// ---- mesh_kernels.hip
// marching tetrahedra on an (nz, ny, nx) lattice; dimensions >= 2, nx * ny * nz < 2^31 (checked by the caller); origin, spacing: host
size_t mesh_workspace_bytes(int nx, int ny, int nz);
int mesh_count(const float* field, int nx, int ny, int nz, float iso, int64_t* counts_dev, void* workspace, hipStream_t st);
int mesh_emit(const float* field, int nx, int ny, int nz, float iso, const float* origin, const float* spacing, void* workspace, int64_t vertex_capacity,
              int64_t face_capacity, float* vertices, float* normals, int32_t* faces, hipStream_t st);
}  // namespace nk
