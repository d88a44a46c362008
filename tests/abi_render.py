"""A stand-in for nerf_amd.ops whose four whole-ray render functions call the argument-list C entry points -- nerf_amd_render_rays,
_warped, _rounds, _ref -- and their own workspace queries directly.  The package itself renders through nerf_amd_render; the four symbols
stay ABI for C callers, and this is the GPU coverage they keep (test_gpu_render_entries, test_gpu_depth_stats).  Same arguments as the ops
functions, without the optional outputs the argument lists have no room for; -> (rgb, depth | None, weights | None -- Ref-NeRF: normal_img
| None --, workspace).  Every other attribute is nerf_amd.ops's."""
import ctypes as C

import torch

from nerf_amd import _lib, ops
from nerf_amd._lib import check, lib
from nerf_amd.ops import _dev, _prop_prec, _ptr, _render_batch, _render_descriptor, _spacing_kind, _stream


def __getattr__(name):
    return getattr(ops, name)


def _buffers(need, dev, N, want_depth, third_shape):
    def out(shape, want=True):
        return torch.empty(shape, dtype=torch.float32, device=dev) if want else None
    return torch.empty(need, dtype=torch.uint8, device=dev), out((N, 3)), out((N,), want_depth), out(third_shape, third_shape is not None)


def _ref(camera):
    return C.byref(camera) if camera is not None else None


def render_rays(packed_prop, packed_mip, precision, rays, z_base, u_strat, u_inv, n_fine, near, far, white_bkg, want_depth=True, want_weights=False,
                camera=None, ray_offset=0, n_rays=None, contract=False, ipe_radius=None, seed=None, rng_ray_offset=0, ipe_dir_norm=None):
    u_strat, u_inv, seed, dev, N = _render_batch(rays, z_base, u_strat, u_inv, seed, n_rays)
    camera, _keep = _render_descriptor(camera, contract, ipe_radius, ipe_dir_norm, seed, rng_ray_offset)
    workspace, rgb, depth, w = _buffers(lib.nerf_amd_render_workspace_bytes(N, n_fine), dev, N, want_depth, (N, n_fine) if want_weights else None)
    check(lib.nerf_amd_render_rays(_ptr(packed_prop), _ptr(packed_mip), _prop_prec(packed_prop, precision, packed_mip), _ptr(rays), _ref(camera), ray_offset,
                                   _ptr(z_base), _ptr(u_strat), _ptr(u_inv), N, n_fine, float(near), float(far), int(white_bkg), _ptr(rgb), _ptr(depth), _ptr(w),
                                   _ptr(workspace), _stream()), "nerf_amd_render_rays")
    return rgb, depth, w, workspace


def render_rays_warped(packed_prop, packed_mip, precision, rays, u_strat, u_inv, n_fine, near, far, white_bkg, *, want_depth=True, want_weights=False,
                       contract=False, ipe_radius=None, seed=None, rng_ray_offset=0, ipe_dir_norm=None, spacing="disparity"):
    rays = _dev(rays, "rays")
    u_strat, u_inv, seed, dev, N = _render_batch(rays, None, u_strat, u_inv, seed, rays.shape[0])
    camera, _keep = _render_descriptor(None, contract, ipe_radius, ipe_dir_norm, seed, rng_ray_offset)
    workspace, rgb, depth, w = _buffers(lib.nerf_amd_render_warped_workspace_bytes(N, n_fine), dev, N, want_depth, (N, n_fine) if want_weights else None)
    check(lib.nerf_amd_render_rays_warped(_ptr(packed_prop), _ptr(packed_mip), _prop_prec(packed_prop, precision, packed_mip), _ptr(rays), _ref(camera), 0,
                                          _ptr(u_strat), _ptr(u_inv), N, int(n_fine), _spacing_kind(spacing), float(near), float(far), int(white_bkg), _ptr(rgb),
                                          _ptr(depth), _ptr(w), _ptr(workspace), _stream()), "nerf_amd_render_rays_warped")
    return rgb, depth, w, workspace


def render_rays_rounds(packed_prop, packed_mip, precision, rays, z_base, n_fine, near, far, white_bkg, *, prop_pnum, seed, rng_ray_offset=0, spacing="linear",
                       contract=False, ipe_radius=None, ipe_dir_norm=None, want_depth=True, want_weights=False):
    rays = _dev(rays, "rays")
    N, kind = rays.shape[0], _spacing_kind(spacing)
    z_base = _dev(z_base, "z_base") if kind == _lib.SPACING_LINEAR else None
    camera, _keep = _render_descriptor(None, contract, ipe_radius, ipe_dir_norm, seed, rng_ray_offset)
    workspace, rgb, depth, w = _buffers(lib.nerf_amd_render_rounds_workspace_bytes(N, int(n_fine), int(prop_pnum), kind), rays.device, N, want_depth,
                                        (N, n_fine) if want_weights else None)
    check(lib.nerf_amd_render_rays_rounds(_ptr(packed_prop), _ptr(packed_mip), _prop_prec(packed_prop, precision, packed_mip), _ptr(rays), _ref(camera), 0,
                                          _ptr(z_base), N, int(n_fine), int(prop_pnum), kind, float(near), float(far), int(white_bkg), _ptr(rgb), _ptr(depth),
                                          _ptr(w), _ptr(workspace), _stream()), "nerf_amd_render_rays_rounds")
    return rgb, depth, w, workspace


def render_rays_ref(packed_prop, packed_ref, precision, rays, z_base, u_strat, u_inv, n_fine, near, far, white_bkg, want_depth=True, cam_dir=None,
                    camera=None, ray_offset=0, n_rays=None, flags=0, seed=None, rng_ray_offset=0, contract=False):
    u_strat, u_inv, seed, dev, N = _render_batch(rays, z_base, u_strat, u_inv, seed, n_rays)
    camera, _keep = _render_descriptor(camera, True if contract else None, None, None, seed, rng_ray_offset)
    cam_dir = _dev(cam_dir, "cam_dir") if cam_dir is not None else None
    workspace, rgb, depth, normal_img = _buffers(lib.nerf_amd_render_ref_workspace_bytes(N, n_fine), dev, N, want_depth, (N,) if cam_dir is not None else None)
    check(lib.nerf_amd_render_rays_ref(_ptr(packed_prop), _ptr(packed_ref), _prop_prec(packed_prop, precision), int(flags), _ptr(rays), _ref(camera), ray_offset,
                                       _ptr(z_base), _ptr(u_strat), _ptr(u_inv), N, n_fine, float(near), float(far), int(white_bkg), _ptr(cam_dir), _ptr(rgb),
                                       _ptr(depth), _ptr(normal_img), _ptr(workspace), _stream()), "nerf_amd_render_rays_ref")
    return rgb, depth, normal_img, workspace
