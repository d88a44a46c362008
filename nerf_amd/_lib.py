"""ctypes binding of libnerf_amd.so (include/nerf_amd.h).  There is NO fallback: if the HIP library
is missing or fails to load, importing this module raises -- the product never silently runs a
torch/CPU substitute."""
import ctypes as C
import os

import torch  # noqa: F401  -- MUST precede the dlopen below: torch bundles its own libamdhip64; loading ours first
#                             would bring up a second HIP runtime that cannot see torch's device allocations.

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NERF_AMD_LIB") or os.path.join(_HERE, "libnerf_amd.so")   # env override: diagnostic builds only

F32, BF16 = 0, 1
BF16_F8 = 2            # NERF_AMD_BF16_F8: bf16 arithmetic, training dumps of the hidden layers in scaled e4m3 (training entry points only)
EXPECTED_VERSION = 125  # nerf_amd_version() of the library these signatures were written against
NET_PROPOSAL, NET_MIP, NET_REF, NET_PROPOSAL_128, NET_MIP_128 = 0, 1, 2, 3, 4
FINE_W128 = 0x200     # layout flag: the fine-network blob is a NET_MIP_128 blob
PROP_W128 = 0x100     # layout flag OR-ed into `precision`: packed_prop is a NET_PROPOSAL_128 blob
ACT_RELU, ACT_IDENTITY, ACT_SOFTPLUS = 0, 1, 2
SPACING_LINEAR, SPACING_DISPARITY = 0, 1   # NERF_AMD_SPACING_*: "disparity" = the Mip-NeRF 360 s-space entry points (nerf_amd_warp*)
SPACINGS = {"linear": SPACING_LINEAR, "disparity": SPACING_DISPARITY}
CONTRACT_GAUSSIAN = 2  # NERF_AMD_CONTRACT_GAUSSIAN: nerf_amd_samples.contract that also contracts the frustum covariance (integrated PE)

c_float_p = C.POINTER(C.c_float)
c_void = C.c_void_p
i64 = C.c_int64


class Samples(C.Structure):
    """struct nerf_amd_samples"""
    _fields_ = [("mode", C.c_int32), ("S", C.c_int32), ("M", C.c_int64), ("pts", c_void), ("pts_stride", C.c_int32),
                ("z_stride", C.c_int32), ("rays", c_void), ("z", c_void), ("z_base", c_void), ("u", c_void),
                ("z_jitter", C.c_float), ("H", C.c_int32), ("W", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("pose", C.c_float * 12), ("contract", C.c_int32), ("ipe", C.c_int32), ("ipe_radius", C.c_float),
                ("ipe_dir_norm", c_void), ("rng_seed", C.c_uint64), ("rng_ray_offset", C.c_int64)]


IMAGE_METRICS_TILE = (16, 64)   # NERF_AMD_IMAGE_METRICS_TILE_H, _TILE_W: the SSIM map tile of nerf_amd_image_metrics
IMAGE_METRICS_SEGMENT_H = 128   # NERF_AMD_IMAGE_METRICS_SEGMENT_H: map rows (a whole number of tiles) that one workgroup walks
MESH_SCAN_STEP_TILES = 4096     # NERF_AMD_MESH_SCAN_STEP_TILES: tiles of 256 lattice points per step of nerf_amd_mesh_count's tile scan
DEPTH_QUANTILES_MAX = 4   # NERF_AMD_DEPTH_QUANTILES_MAX: quantiles per nerf_amd_ray_depth_stats / nerf_amd_render call


class RenderRequest(C.Structure):
    """struct nerf_amd_render_request (a zero-filled instance has every optional field off; ``size`` is set on construction)"""
    _fields_ = [("size", C.c_size_t), ("packed_prop", c_void), ("packed_fine", c_void), ("precision", C.c_int32), ("ref", C.c_int32),
                ("ref_flags", C.c_int32), ("white_bkg", C.c_int32), ("rays", c_void), ("camera", C.POINTER(Samples)), ("ray_offset", C.c_int64),
                ("z_base", c_void), ("u_strat", c_void), ("u_inv", c_void), ("N", C.c_int64), ("n_fine", C.c_int32), ("prop_pnum", C.c_int32),
                ("spacing", C.c_int32), ("near", C.c_float), ("far", C.c_float), ("n_quantiles", C.c_int32),
                ("quantiles", C.c_float * DEPTH_QUANTILES_MAX), ("cam_dir", c_void), ("rgb", c_void), ("depth", c_void), ("weights", c_void),
                ("normal_img", c_void), ("opacity", c_void), ("depth_q", c_void), ("fine_depths", c_void),
                # appended behind the first layout (200 bytes, which the library still accepts): the empty-ray skip
                ("skip_min_optical_depth", C.c_double), ("row_of_ray", c_void), ("n_alive", C.POINTER(C.c_int64))]

    def __init__(self, **fields):
        super().__init__(**fields)
        self.size = C.sizeof(RenderRequest)


# name -> (restype, argtypes); mirrors include/nerf_amd.h one to one (tests check the two agree)
SIGNATURES = {
    "nerf_amd_last_error": (C.c_char_p, []),
    "nerf_amd_version": (C.c_int, []),
    "nerf_amd_device_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nerf_amd_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "nerf_amd_pack_weights": (C.c_int, [C.c_int, C.c_int, C.POINTER(c_void), C.POINTER(c_void), C.c_int, c_void, c_void]),
    "nerf_amd_proposal_forward": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), c_void, c_void]),
    "nerf_amd_mip_forward": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), c_void, c_void]),
    "nerf_amd_direction_table": (C.c_int, [c_void, i64, c_void, c_void]),
    "nerf_amd_mip_forward_composite": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), C.c_int, C.c_float, C.c_float, c_void, c_void, c_void,
                                                 c_void]),
    "nerf_amd_ref_forward": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), C.c_int, c_void, c_void, c_void]),
    "nerf_amd_ref_forward_train": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), C.c_int, c_void, c_void, c_void, c_void]),
    "nerf_amd_positional_encoding": (C.c_int, [c_void, i64, C.c_int, c_void, c_void]),
    "nerf_amd_ipe_feature": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_ipe_feature_contracted": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_ipe_feature_gaussian": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_cone_parameters": (C.c_int, [c_void, i64, C.c_int, C.c_float, c_void, c_void, c_void, c_void]),
    "nerf_amd_dirs_norm": (C.c_int, [c_void, i64, c_void, c_void]),
    "nerf_amd_generate_rays": (C.c_int, [c_float_p, C.c_int, C.c_int, C.c_float, C.c_float, i64, i64, c_void, c_void]),
    "nerf_amd_length2pts": (C.c_int, [c_void, c_void, i64, C.c_int, c_void, c_void]),
    "nerf_amd_sigma_to_weights": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_max_blur": (C.c_int, [c_void, i64, C.c_int, C.c_float, c_void, c_void]),
    "nerf_amd_inverse_sample": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nerf_amd_sample_pdf": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nerf_amd_pixel_rays": (C.c_int, [c_float_p, C.c_float, C.c_float, c_void, i64, c_void, c_void]),
    "nerf_amd_sample_training_rays": (C.c_int, [c_void, c_void, i64, c_float_p, C.c_float, C.c_float, C.c_float, C.c_float, i64, C.c_int, C.c_uint64,
                                               c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_sample_training_rays_dev": (C.c_int, [c_void, c_void, i64, c_void, C.c_float, C.c_float, C.c_float, C.c_float, i64, C.c_int, c_void,
                                                   c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_sample_scene_rays": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                            C.c_float, C.c_float, i64, C.c_int, C.c_uint64, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_generate_rays_camera": (C.c_int, [c_float_p, C.c_int, C.c_int, c_float_p, i64, i64, c_void, c_void]),
    "nerf_amd_sample_scene_rays_camera": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_int, c_void,
                                                   C.c_float, C.c_float, i64, C.c_int, C.c_uint64, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_philox_uniforms": (C.c_int, [c_void, i64, C.c_int, C.c_uint64, c_void, c_void]),
    "nerf_amd_philox_stream": (C.c_int, [c_void, i64, C.c_int, C.c_uint64, c_void, i64, C.c_int, c_void]),
    "nerf_amd_advance_seed": (C.c_int, [c_void, c_void]),
    "nerf_amd_stratified_points": (C.c_int, [c_void, c_void, c_void, C.c_float, i64, C.c_int, c_void, c_void, c_void]),
    "nerf_amd_resample": (C.c_int, [c_void, c_void, c_void, c_void, C.c_float, c_void, C.c_int, c_void, i64, C.c_int,
                                    C.c_int, C.c_int, C.c_float, C.c_uint64, i64, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_composite": (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_int, i64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_float, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_train_dump_rows_mask_partials": (i64, []),
    "nerf_amd_train_dump_rows_mask": (C.c_int, [c_void, C.c_int, C.c_int, i64, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nerf_amd_render_ref_workspace_bytes": (C.c_size_t, [i64, C.c_int]),
    "nerf_amd_render_rays_ref": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, C.POINTER(Samples), i64, c_void, c_void, c_void, i64, C.c_int,
                                          C.c_float, C.c_float, C.c_int, c_void, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_encode_rows": (C.c_int, [c_void, C.c_int, i64, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_merge_depths": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_merge_depths_order": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nerf_amd_coarse_grad_select": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_mfma_stream": (C.c_int, [C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_weighted_dot_loss": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nerf_amd_weighted_dot_loss_backward": (C.c_int, [c_void, c_void, c_void, c_void, i64, C.c_int, C.c_float, c_void, c_void, c_void, c_void]),
    "nerf_amd_distortion_loss": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nerf_amd_distortion_loss_backward": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void]),
    "nerf_amd_interlevel_loss": (C.c_int, [c_void, c_void, c_void, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void, c_void]),
    "nerf_amd_interlevel_loss_backward": (C.c_int, [c_void, c_void, c_void, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nerf_amd_get_bounds": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_train_dump_bytes": (C.c_size_t, [C.c_int, C.c_int, i64]),
    "nerf_amd_proposal_forward_train": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), c_void, c_void, c_void]),
    "nerf_amd_mip_forward_train": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), c_void, c_void, c_void]),
    "nerf_amd_train_dump_to_rows": (C.c_int, [c_void, C.c_int, C.c_int, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_relu_mask": (C.c_int, [c_void, c_void, C.c_int, i64, c_void]),
    "nerf_amd_relu_mask_bias_partials": (i64, [C.c_int, i64, C.c_int]),
    "nerf_amd_relu_mask_bias": (C.c_int, [c_void, c_void, C.c_int, i64, C.c_int, c_void, c_void]),
    "nerf_amd_packed_backward_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "nerf_amd_pack_weights_backward": (C.c_int, [C.c_int, C.c_int, C.POINTER(c_void), C.c_int, c_void, c_void]),
    "nerf_amd_proposal_backward_chain": (C.c_int, [c_void, C.c_int, c_void, i64, c_void, c_void, c_void]),
    "nerf_amd_mip_backward_chain": (C.c_int, [c_void, C.c_int, c_void, c_void, i64, c_void, c_void, c_void]),
    "nerf_amd_weight_grads_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, i64]),
    "nerf_amd_proposal_weight_grads": (C.c_int, [C.c_int, i64, c_void, c_void, C.POINTER(c_void), C.POINTER(c_void), c_void, c_void]),
    "nerf_amd_mip_weight_grads": (C.c_int, [C.c_int, i64, c_void, c_void, C.POINTER(c_void), C.POINTER(c_void), C.POINTER(c_void),
                                           C.POINTER(c_void), c_void, c_void]),
    "nerf_amd_ref_forward_train_dump": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), C.c_int, c_void, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_ref_forward_train_dump_rng": (C.c_int, [c_void, C.c_int, C.POINTER(Samples), C.c_int, C.c_uint64, c_void, C.c_float, c_void, c_void, c_void,
                                                      c_void, c_void]),
    "nerf_amd_philox_normal": (C.c_int, [c_void, i64, C.c_uint64, c_void, C.c_float, i64, c_void]),
    "nerf_amd_density_grad_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, i64]),
    "nerf_amd_density_grad": (C.c_int, [C.c_int, c_void, C.c_int, i64, c_void, c_void, C.c_int, c_void, C.c_int, c_void, c_void, c_void]),
    "nerf_amd_ref_backward_workspace_bytes": (C.c_size_t, [C.c_int, i64]),
    "nerf_amd_ref_backward": (C.c_int, [c_void, C.c_int, C.c_int, i64, c_void, c_void, c_void, C.c_int, c_void, C.c_int, c_void, C.POINTER(c_void),
                                       C.POINTER(c_void), c_void, c_void]),
    "nerf_amd_adam_step": (C.c_int, [C.POINTER(c_void), C.POINTER(c_void), C.POINTER(c_void), C.POINTER(c_void), C.POINTER(i64), C.c_int, c_void,
                                    C.c_double, c_void, C.c_double, C.c_double, C.c_double, C.c_float, c_void]),
    "nerf_amd_sigma_to_weights_backward": (C.c_int, [c_void, c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nerf_amd_composite_backward": (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_int, i64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                              C.c_float, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_max_blur_backward": (C.c_int, [c_void, c_void, i64, C.c_int, c_void, c_void]),
    "nerf_amd_get_bounds_backward": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_render_workspace_bytes": (C.c_size_t, [i64, C.c_int]),
    "nerf_amd_render_rays": (C.c_int, [c_void, c_void, C.c_int, c_void, C.POINTER(Samples), i64, c_void, c_void, c_void, i64,
                                       C.c_int, C.c_float, C.c_float, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_warp_depths": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, c_void, c_void, c_void]),
    "nerf_amd_warped_stratified": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_uint64, i64, C.c_int, C.c_float, C.c_float, c_void, c_void, c_void, c_void]),
    "nerf_amd_warped_resample": (C.c_int, [c_void, c_void, c_void, C.c_int, c_void, i64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                           C.c_float, C.c_uint64, i64, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_render_warped_workspace_bytes": (C.c_size_t, [i64, C.c_int]),
    "nerf_amd_render_rays_warped": (C.c_int, [c_void, c_void, C.c_int, c_void, C.POINTER(Samples), i64, c_void, c_void, i64, C.c_int, C.c_int,
                                              C.c_float, C.c_float, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_render_rounds_workspace_bytes": (C.c_size_t, [i64, C.c_int, C.c_int, C.c_int]),
    "nerf_amd_render_rays_rounds": (C.c_int, [c_void, c_void, C.c_int, c_void, C.POINTER(Samples), i64, c_void, i64, C.c_int, C.c_int, C.c_int,
                                              C.c_float, C.c_float, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_ray_depth_stats": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, C.c_int, i64, C.c_int, C.c_int, c_float_p, C.c_int, C.c_float, C.c_float,
                                          c_void, c_void, c_void]),
    "nerf_amd_render_request_workspace_bytes": (C.c_size_t, [C.POINTER(RenderRequest)]),
    "nerf_amd_render": (C.c_int, [C.POINTER(RenderRequest), c_void, c_void]),
    "nerf_amd_ray_alive_workspace_bytes": (C.c_size_t, [i64]),
    "nerf_amd_ray_alive": (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_int, i64, C.c_int, C.c_double, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_gather_rows": (C.c_int, [c_void, i64, c_void, i64, C.c_int, c_void, c_void]),
    "nerf_amd_gemm_workspace_bytes": (C.c_size_t, [i64, i64, i64]),
    "nerf_amd_gemm": (C.c_int, [C.c_int, i64, i64, i64, c_void, i64, i64, c_void, i64, i64, c_void, i64, c_void, C.c_int, c_void, i64, c_void, c_void]),
    "nerf_amd_sigmoid_backward": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, c_void, i64, c_void]),
    "nerf_amd_ref_dir_inputs": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, c_void, c_void, i64, c_void, c_void]),
    "nerf_amd_ref_dir_inputs_backward": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, c_void, c_void, i64, c_void, i64, c_void, i64, c_void]),
    "nerf_amd_ref_combine": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, c_void, c_void]),
    "nerf_amd_ref_combine_backward": (C.c_int, [c_void, i64, c_void, i64, c_void, i64, i64, C.c_int, c_void, i64, c_void, i64, c_void]),
    "nerf_amd_positional_encoding_backward": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, C.c_int, c_void, c_void]),
    "nerf_amd_contract_positions": (C.c_int, [c_void, i64, i64, c_void, i64, c_void, c_void]),
    "nerf_amd_add_rows": (C.c_int, [c_void, i64, c_void, i64, i64, C.c_int, c_void]),
    "nerf_amd_rows_gemm": (C.c_int, [i64, i64, i64, c_void, i64, c_void, i64, i64, c_void, C.c_int, c_void, i64, C.c_int, c_void]),
    "nerf_amd_rows_to_bf16": (C.c_int, [c_void, i64, i64, i64, C.c_int, C.c_int, c_void, i64, c_void]),
    "nerf_amd_image_metrics_workspace_bytes": (C.c_size_t, [i64, C.c_int, C.c_int, C.c_int]),
    "nerf_amd_image_metrics": (C.c_int, [c_void, c_void, i64, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    "nerf_amd_mesh_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "nerf_amd_mesh_count": (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nerf_amd_mesh_emit": (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_float_p, c_float_p, c_void, i64, i64, c_void, c_void, c_void, c_void]),
}


# additive entry points that a library named by NERF_AMD_LIB may predate
ADDED_AFTER_125 = ("nerf_amd_direction_table", "nerf_amd_render_rounds_workspace_bytes", "nerf_amd_render_rays_rounds",
                   "nerf_amd_ipe_feature_gaussian", "nerf_amd_ray_depth_stats", "nerf_amd_render_request_workspace_bytes", "nerf_amd_render",
                   "nerf_amd_ray_alive_workspace_bytes", "nerf_amd_ray_alive", "nerf_amd_gather_rows", "nerf_amd_generate_rays_camera",
                   "nerf_amd_sample_scene_rays_camera", "nerf_amd_image_metrics_workspace_bytes", "nerf_amd_image_metrics",
                   "nerf_amd_mesh_workspace_bytes", "nerf_amd_mesh_count", "nerf_amd_mesh_emit")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "nerf_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C nerf_amd/csrc`). There is no CPU/torch fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if name in ADDED_AFTER_125 and os.environ.get("NERF_AMD_LIB") and not hasattr(lib, name):
            continue                            # a diagnostic build of an older tree (A/B runs against a parent library)
        fn = getattr(lib, name)                 # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    got = lib.nerf_amd_version()
    if got != EXPECTED_VERSION and not os.environ.get("NERF_AMD_LIB"):      # a stale git-ignored .so would be called with shifted arguments
        raise ImportError("nerf_amd: %s is ABI version %d, this package expects %d -- rebuild it (`make -C nerf_amd/csrc`)" % (LIB_PATH, got, EXPECTED_VERSION))
    return lib


lib = _load()


class NerfAmdError(RuntimeError):
    pass


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib.nerf_amd_last_error()
        raise NerfAmdError("%s failed (%d): %s" % (what or "nerf_amd call", rc, msg.decode() if msg else "?"))
