"""Host-side mirror of the reference's ``nerf/procedures.py``: ``render_image`` with the reference's
signature, tile order, RNG protocol and return dict -- but the whole image goes through the HIP
pipeline in four launches instead of a Python loop over 2500-ray tiles."""
import argparse
from collections.abc import Iterable
from typing import Optional

import torch

from . import ops
from .addtional import ProposalNetwork
from .nerf_base import NeRF

POSSIBLE_PATCH_SIZE = [50, 40, 60, 30]
RENDER_COARSE_PNUM = 64


def get_patch_size(image_size):
    """First patch size in (50,40,60,30) that divides the width (procedures.py:24-31); None when there is
    none (the reference raises UnboundLocalError there; this build then renders the image un-tiled)."""
    for p in POSSIBLE_PATCH_SIZE:
        if image_size[1] % p == 0:
            return p, (image_size[0] // p, image_size[1] // p)
    return None, None


def _draw_uniforms(H, W, sample_num, sz, patch_num, device, rng):
    """Uniforms for every ray, in TILE order when tiling applies.
    rng='reference': per tile one (sz,sz,64) draw then one (sz*sz, sample_num+1) draw from the CPU default
    generator -- exactly the reference's order (procedures.py:65, utils.py:115), so a seeded run reproduces it;
    rng='device': two draws on the device generator (fast path, used by bench.py)."""
    if rng == "device":
        n = (patch_num[0] * patch_num[1] * sz * sz) if sz else H * W
        return (torch.rand((n, RENDER_COARSE_PNUM), device=device), torch.rand((n, sample_num + 1), device=device))
    if sz is None:
        return torch.rand((H * W, RENDER_COARSE_PNUM)).to(device), torch.rand((H * W, sample_num + 1)).to(device)
    n_tiles = patch_num[0] * patch_num[1]
    u1 = torch.empty((n_tiles, sz * sz, RENDER_COARSE_PNUM))
    u2 = torch.empty((n_tiles, sz * sz, sample_num + 1))
    for t in range(n_tiles):
        u1[t] = torch.rand((sz, sz, RENDER_COARSE_PNUM)).view(-1, RENDER_COARSE_PNUM)
        u2[t] = torch.rand((sz * sz, sample_num + 1))
    return u1.view(-1, RENDER_COARSE_PNUM).to(device), u2.view(-1, sample_num + 1).to(device)


# rays per chunk of the layer-by-layer route (the reference tiles an image the same way, procedures.py:53-56)
GENERIC_CHUNK_RAYS = 4096


def _render_rays_by_calls(network, prop_net, rays, z_base, u_strat, u_inv, sample_num, near, far, white_bkg, render_depth, chunk: Optional[int] = None,
                          is_ref_model: bool = False, cam_dir=None, seed: Optional[int] = None, ray_offset: int = 0, contract: bool = False,
                          ipe_radius: Optional[float] = None, ipe_dir_norm=None, *, spacing: str = "linear", prop_rounds: int = 1,
                          prop_pnum: Optional[int] = None, ipe_cov: str = "metric", skip_min_optical_depth: Optional[float] = None,
                          depth_quantiles=None, render_opacity: bool = False):
    """The tile body of procedures.py:62-85 as the reference writes it -- stratified depths, ProposalNetwork.forward, get_weights,
    maxBlurFilter, inverseSample, NeRF.length2pts, network.forward, NeRF.render -- on chunks of rays: the route of networks the fused
    render entry (nerf_amd_render_rays) has no packed layout for.  Every call is a HIP kernel of this package; uniforms that were not
    given are the render kernels' own Philox streams for `seed` and the chunk's global ray indices (ops.philox_stream): the image of a
    seeded render does not depend on whether a network runs fused or layer by layer.
    ``spacing="disparity"`` (Mip-NeRF 360's s-space, include/nerf_amd.h): the coarse draw and the resampling happen in the normalised
    distance s, everything else -- weights, coarseFineMerge (W is monotone: the order is that of s), encodings, compositing -- on the metric
    depths W(s); the depth is W^-1 of the expected metric depth.
    ``prop_rounds=2`` (Mip-NeRF 360's two proposal rounds; Philox uniforms only): between the proposal pass and the fine resampling,
    ``prop_pnum`` sorted depths are resampled from the first histogram, the proposal network is evaluated there and the fine depths are
    drawn from that second histogram.  The ray's inverse-CDF stream then has prop_pnum + sample_num + 1 columns: the first prop_pnum feed
    the second round, the rest the fine resampling.
    ``ipe_cov`` (with ``ipe_radius`` and ``contract``): "contracted" = the frustum covariance goes through the contraction with its mean
    (MipNeRF.forward_rays); the proposal passes contract positions as before.
    ``depth_quantiles`` / ``render_opacity`` (render_image's): ops.ray_depth_stats of NeRF.render's weights and the depth row it
    composited -- the sample_num + 1 sorted depths with their closing edge, Ref-NeRF the merged open row -- normalised like the depth;
    when either is set a dict {"depth_q" (N,Q) | None, "opacity" (N,) | None} follows the three results.
    ``skip_min_optical_depth`` (render_image's ``skip_empty`` as D_min): the empty-ray skip of include/nerf_amd.h on this route --
    ops.ray_alive on the histogram the fine depths were drawn from, the fine network on the alive rays only (torch indexing gathers its
    inputs and scatters its rows into zeros: plumbing), compositing on all rays; the same image as the fused routes.  The dict then
    follows too and also holds "row_of_ray" (N,) int32 and "n_alive"."""
    from .mip_methods import maxBlurFilter
    ops.ipe_contract(contract, ipe_radius, ipe_cov, "nerf_amd.render_image")
    quantiles = ops.depth_quantiles(depth_quantiles, "nerf_amd.render_image")
    want_stats = bool(quantiles) or bool(render_opacity)
    skip_dmin = ops.skip_threshold(None, skip_min_optical_depth, "nerf_amd.render_image")
    from .utils import inverseSample
    N = rays.shape[0]
    chunk = GENERIC_CHUNK_RAYS if chunk is None else chunk
    rgb = torch.empty((N, 3), dtype=torch.float32, device=rays.device)
    depth = torch.empty((N,), dtype=torch.float32, device=rays.device) if render_depth else None
    normal_px = torch.empty((N,), dtype=torch.float32, device=rays.device) if cam_dir is not None else None
    stats = {"depth_q": torch.empty((N, len(quantiles)), dtype=torch.float32, device=rays.device) if quantiles else None,
             "opacity": torch.empty((N,), dtype=torch.float32, device=rays.device) if render_opacity else None}
    if skip_dmin:
        stats.update(row_of_ray=torch.empty((N,), dtype=torch.int32, device=rays.device), n_alive=0)
        if ipe_radius is not None and ipe_dir_norm is None:
            ipe_dir_norm = ops.dirs_norm(rays)                                      # the norm of the whole ray list, not of the alive rays
    resolution = (far - near) / sample_num                                           # procedures.py:57
    warped = _check_spacing(spacing, near, far)
    for s in range(0, N, chunk):
        r = rays[s: s + chunk].contiguous()
        n = r.shape[0]
        u1 = u_strat[s: s + n] if u_strat is not None else ops.philox_stream((n, RENDER_COARSE_PNUM), seed, ray_offset + s, strat=True, device=rays.device)
        if prop_rounds == 2:
            u12 = ops.philox_stream((n, prop_pnum + sample_num + 1), seed, ray_offset + s, device=rays.device)
            u_mid, u2 = u12[:, :prop_pnum].contiguous(), u12[:, prop_pnum:]
        else:
            u2 = u_inv[s: s + n] if u_inv is not None else ops.philox_stream((n, sample_num + 1), seed, ray_offset + s, device=rays.device)
        if warped:
            s_c, z, pts = ops.warped_stratified(r, u1.contiguous(), near, far, spacing=spacing)
        else:
            z, pts = ops.stratified_points(r, z_base, u1.contiguous(), resolution)  # :65-66
        density = prop_net.forward(pts, contract=True) if contract else prop_net.forward(pts)
        prop_w = maxBlurFilter(ProposalNetwork.get_weights(density, z, r[:, 3:]), 0.01)
        if prop_rounds == 2:                                                         # the second histogram: the same network at depths drawn from the first
            if warped:
                s_c, _ = inverseSample(prop_w, s_c, prop_pnum, sort=True, u=u_mid)
                z, pts = ops.warp_depths(s_c, near, far, r, spacing=spacing)
            else:
                z, _ = inverseSample(prop_w, z, prop_pnum, sort=True, u=u_mid)
                pts = NeRF.length2pts(r, z)[..., :3].contiguous()
            density = prop_net.forward(pts, contract=True) if contract else prop_net.forward(pts)
            prop_w = maxBlurFilter(ProposalNetwork.get_weights(density, z, r[:, 3:]), 0.01)
        if warped:                                                                   # resample in s, then back to metric depths
            s_f, _ = inverseSample(prop_w, s_c, sample_num + 1, sort=True, u=u2.contiguous())
            fine = ops.warp_depths(s_f, near, far, spacing=spacing)[0]
        else:
            fine, _ = inverseSample(prop_w, z, sample_num + 1, sort=True, u=u2.contiguous())
        normal = None
        edges = fine                                                                 # the depth row of the quantiles: the closing edge still on it
        alive = None                                                                 # the empty-ray skip: the alive rays' indices in this chunk
        if skip_dmin:
            row, alive, n_alive = ops.ray_alive(density.reshape(n, -1), z, r, min_optical_depth=skip_dmin)
            stats["row_of_ray"][s: s + n] = torch.where(row >= 0, row + stats["n_alive"], row)
            stats["n_alive"] += n_alive

        def on_alive(run, *full):
            """run(*inputs) on the alive rays' rows of `full`; its outputs scattered into zeros of the chunk's size (dense: run(*full))"""
            if alive is None:
                return run(*full)
            if alive.numel() == 0:
                return None
            return tuple(torch.zeros((n,) + o.shape[1:], dtype=o.dtype, device=o.device).index_copy_(0, alive, o) for o in run(*[t[alive].contiguous() for t in full]))
        if is_ref_model:                                                             # :71-74
            samples, fine = NeRF.coarseFineMerge(r, z, fine)
            edges = fine                                                             # (Ref-NeRF: the merged row, open)
            out = on_alive(lambda sm: tuple(network.forward(sm, contract=True) if contract else network.forward(sm)), samples)
            S_all = fine.shape[-1]
            rgbo, normal = out if out is not None else (torch.zeros((n, S_all, 4), device=r.device), torch.zeros((n, S_all, 3), device=r.device))
            rgbo[..., -1] = torch.nn.functional.softplus(rgbo[..., -1] + 0.5)
        elif ipe_radius is not None:                                                  # frusta between the sample_num + 1 sorted depths
            out = on_alive(lambda rr, ff: (network.forward_rays(rr, ff, sample_num, ipe_radius=ipe_radius, ipe_dir_norm=ipe_dir_norm, contract=contract, ipe_cov=ipe_cov),),
                           r, fine.contiguous())
            rgbo = out[0] if out is not None else torch.zeros((n, sample_num, 4), device=r.device)
            fine = fine[..., :-1].contiguous()
        else:
            fine = fine[..., :-1].contiguous()
            out = on_alive(lambda pp: (network.forward(pp, contract=True) if contract else network.forward(pp),), NeRF.length2pts(r, fine))
            rgbo = out[0] if out is not None else torch.zeros((n, sample_num, 4), device=r.device)
        part, weights, extras = NeRF.render(rgbo, fine, r[:, 3:], white_bkg=white_bkg, density_act=torch.nn.functional.relu,
                                            render_depth=((0.0, 1.0) if warped else (near, far)) if render_depth else None,
                                            normal_info=(normal, cam_dir) if cam_dir is not None else None)
        rgb[s: s + n] = part
        if want_stats:
            dq, op = ops.ray_depth_stats(weights, edges.contiguous(), r, quantiles=quantiles, near=0.0 if warped else near, far=1.0 if warped else far,
                                         want_opacity=bool(render_opacity))
            if quantiles:
                stats["depth_q"][s: s + n] = ops.warp_depths(dq, near, far, inverse=True, spacing=spacing)[0] if warped else dq
            if render_opacity:
                stats["opacity"][s: s + n] = op
        if render_depth:
            d = extras["depth_img"].reshape(n, 1)
            depth[s: s + n] = (ops.warp_depths(d, near, far, inverse=True, spacing=spacing)[0] if warped else d).reshape(-1)
        if cam_dir is not None:
            normal_px[s: s + n] = extras["normal_img"].reshape(-1)
    if want_stats or skip_dmin:
        return rgb, depth, normal_px, stats
    return rgb, depth, normal_px


def _render_route(is_ref_model: bool, generic: bool, warped: bool, prop_rounds: int, prop_pnum: int) -> str:
    """Which way render_image renders its rays.  ``generic``: a network the fused kernels have no packed layout for (hidden width > 256,
    > 10 octaves); ``warped``: disparity spacing.  (Ref-NeRF with two rounds or with the integrated PE is refused before this is asked.)

        generic   prop_rounds          fine network   spacing      route      renders through
        yes       any                  any            any          "calls"    _render_rays_by_calls: the tile body call by call, layer by layer
        no        2, prop_pnum 3..256  MipNeRF        any          "rounds"   ops.render_rays_rounds
        no        2, other prop_pnum   MipNeRF        any          "calls"    (no fused entry point for that histogram size)
        no        1                    Ref-NeRF       linear       "ref"      ops.render_rays_ref
        no        1                    Ref-NeRF       disparity    "calls"    (the fused Ref-NeRF entry point has no disparity twin)
        no        1                    MipNeRF        disparity    "warped"   ops.render_rays_warped
        no        1                    MipNeRF        linear       "plain"    ops.render_rays

    Every route draws from the same uniforms -- the tensors of rng="reference" / "device", or the Philox streams of the global ray index --
    so the image does not depend on the route."""
    if generic:
        return "calls"
    if prop_rounds == 2:
        return "rounds" if ops.ROUNDS_PNUM_MIN <= prop_pnum <= ops.ROUNDS_PNUM_MAX else "calls"
    if is_ref_model:
        return "calls" if warped else "ref"
    return "warped" if warped else "plain"


def _check_spacing(spacing, near, far) -> bool:
    """True for "disparity", False for "linear" (which must not reach any of the warped code); anything else raises."""
    if spacing == "linear":
        return False
    if spacing != "disparity":
        raise ValueError("nerf_amd: spacing must be 'linear' or 'disparity' (got %r)" % (spacing,))
    if not 0.0 < float(near) < float(far):
        raise ValueError("nerf_amd: spacing='disparity' needs 0 < near < far")
    return True


_COARSE_DEPTHS = {}


def _coarse_depths(near, far, dev) -> torch.Tensor:
    """the coarse depths of render_image, torch.linspace(near, far, 64) evaluated on the CPU (the reference's bits) and uploaded ONCE per
    (near, far, device): a constant that every later call reads -- a test set's views do not upload it again (and do not wait for it)"""
    key = (float(near), float(far), str(dev), RENDER_COARSE_PNUM)
    z = _COARSE_DEPTHS.get(key)
    if z is None:
        if len(_COARSE_DEPTHS) >= 64:
            _COARSE_DEPTHS.clear()
        z = _COARSE_DEPTHS[key] = torch.linspace(near, far, RENDER_COARSE_PNUM, device="cpu").to(dev)
    return z


def render_image(network: NeRF, prop_net: ProposalNetwork, render_pose: torch.Tensor, image_size, focal,
                 near: float, far: float, sample_num: int = 128, white_bkg: bool = False, render_depth=False,
                 render_normal=False, rng: str = "philox", contract: bool = False, ipe=False, seed: Optional[int] = None,
                 _shard=None, *, spacing: str = "linear", prop_rounds: int = 1, prop_pnum: Optional[int] = None, ipe_cov: str = "metric",
                 skip_empty: Optional[float] = None, camera=None, depth_quantiles=None, render_opacity: bool = False) -> dict:
    """Whole-image inference (procedures.py:34-97) -> {"rgb" (3,H,W) [, "depth_img" (3,H,W)]} on
    ``render_pose.device``.  The caller provides ``no_grad``/``eval()`` like for the reference.
    ``rng``, ``contract`` and ``ipe`` are additions.  ``rng``: where the stratified / inverse-CDF uniforms come from --
      "philox" (default): drawn INSIDE the kernels, Philox4x32-10 keyed by one 62-bit seed taken from torch's CPU generator (so
                 ``torch.manual_seed`` makes a render reproducible); no uniform tensor exists, the drop-in call runs at the kernels' rate;
      "reference": the reference's own stream -- per tile one (sz,sz,64) then one (sz*sz, n+1) draw from the CPU default generator
                 (procedures.py:65, utils.py:115) copied to the device: a seeded run reproduces the reference's image bit for bit in
                 its uniforms (0.5 GB over PCIe per 800x800 image: ~1.4 M rays/s);
      "device":  two torch.rand draws on the device generator.
    ``seed`` (philox mode): the Philox key itself instead of a draw from the CPU generator.  ``_shard = (start, end)`` (internal:
    nerf_amd.parallel.render_image_sharded) renders only those rays of the image's TILE-ORDERED ray list -- every uniform is a pure
    function of (key, global index in that list), so shards reproduce the single-process image bit for bit -- and returns the per-ray
    outputs ``{"rgb_rays", "depth_rays", "normal_rays", "range", "to_image"}`` instead of images.
    ``contract=True`` applies the Mip-NeRF 360 scene contraction to every sample
    position before the networks encode it (unbounded scenes, BASELINE config 5; not available for Ref-NeRF).  ``ipe`` (BASELINE
    config 3): the fine network reads the integrated positional encoding of the conical frustum between consecutive fine depths
    (mip_methods.py:15-58: [mu | ipe_feature]) instead of the point encoding; True = the pixel radius 2/sqrt(12) pixel widths of
    Mip-NeRF, a float = that radius.  The reference holds `ipe_feature` but never calls it: its use inside the loop is this build's
    definition (oracle.render_rays(ipe_radius=...)), parity of the function itself is pinned by golden G12.
    ``spacing`` (keyword-only; an addition for unbounded scenes, BASELINE config 5): "linear" (default) = the reference's depths, spaced
    evenly between near and far; "disparity" = Mip-NeRF 360's normalised distance s (include/nerf_amd.h): the 64 coarse samples and the
    inverse-CDF resampling are uniform in 1/z, so near = 0.2, far = 1e6 spends its samples near the camera and still reaches the
    background; ``depth_img`` is then W^-1 of the expected depth, in [0, 1].  The compiled-shape MipNeRF goes through
    nerf_amd_render_rays_warped; Ref-NeRF and layer-by-layer networks through the call-by-call route, on the same Philox streams.
    The disparity resampling kernel keeps four rays' rows in 64 KiB of LDS: ``sample_num`` <= 623 under "disparity" (a larger count
    raises; "linear" takes up to 1023).
    ``prop_rounds`` (keyword-only; an addition): 2 = Mip-NeRF 360's two proposal rounds, for a model trained with
    ``TrainStep(prop_rounds=2)``: ``prop_pnum`` (default: the 64 coarse samples' count) sorted depths are resampled from the first proposal
    histogram, the same proposal network is evaluated there, and the fine depths are drawn from that second histogram.  Compiled-shape
    networks with 3 <= prop_pnum <= 256 go through nerf_amd_render_rays_rounds under both spacings (profiles/two_round_render_summary.md);
    layer-by-layer networks and other histogram sizes take the call-by-call route, which computes the same image on the same streams;
    ``rng="philox"`` only -- each ray's inverse-CDF stream simply has prop_pnum more columns, still a pure function of (seed, global ray
    index), so shards reproduce the whole image bit for bit; not available for Ref-NeRF.
    ``ipe_cov`` (keyword-only; an addition, with ``ipe`` and ``contract=True`` only): "metric" (default) contracts the frustum MEAN and
    leaves the covariance in metric space; "contracted" pushes the whole Gaussian through the linearised contraction like Mip-NeRF 360
    (eq. 11-14: mu' = f(mu), Sigma' = J Sigma J^T), so that the attenuation exp(-0.5 4^l var) is measured in the coordinates the mean
    lives in and the far background keeps its low frequencies.  Every route -- fused, two rounds, disparity,
    layer by layer, sharded -- computes the same function; frusta inside the unit ball are the same bits under both.
    ``depth_quantiles`` (keyword-only; an addition): up to 4 values q in (0, 1) -> ``result["depth_quantiles"]`` (Q,H,W), the depth at
    which a ray's cumulative weight reaches q -- (0.5,) is the median ray-termination depth Mip-NeRF 360 shows, which a little weight far
    out does not drag through empty space like the expected depth.  Definition (include/nerf_amd.h, tests/depth_stats_ref.py): with the
    fine pass's weights w_s and sorted depths t_s = z_s |d|, C summed in fp64, k the first interval at which C reaches q,
    D_q = t_k + (q - C_k) / w_k (t_{k+1} - t_k), normalised like ``depth_img`` ((D - near) / (far - near); W^-1(D) under "disparity").
    The mass is ABSOLUTE, not renormalised: a ray that never accumulates q (it leaves the scene with opacity < q) reports its far edge.
    ``render_opacity`` (keyword-only; an addition): ``result["opacity_img"]`` (H,W), the accumulated opacity sum_s w_s -- masks, RGBA
    export, background replacement.  Both come from one more kernel on what compositing leaves in the workspace, on every route; with
    neither set the call and the dict are exactly what they were.  A ``_shard`` call adds "depth_q_rays" (n,Q) and "opacity_rays" (n,).
    ``skip_empty`` (keyword-only; an addition, off by default): an opacity tau in (0, 1) -- the fine network is not run on the rays whose
    PROPOSAL histogram (the one the fine depths are drawn from) has an opacity below tau, i.e. an optical depth D < -log1p(-tau)
    (include/nerf_amd.h, tests/skip_empty_ref.py).  Every output equals the dense render's with the fine network's rows of the skipped rays
    replaced by zeros, bit for bit: an alive pixel is the dense pixel; a skipped MipNeRF pixel is the background colour with zero weights,
    opacity 0 and the far edge as quantile depth (Ref-NeRF composites softplus(sigma + 0.5): a zero row is a constant density with zero colour
    there, not the background).  This is an APPROXIMATION of the image: its error is the fine opacity of the rays the proposal network calls
    empty, so it suits models whose proposal network was trained to bound the fine weights.  The result gains "alive_img" (H,W) bool and
    "alive_fraction" (a Python float); a ``_shard`` call adds "alive_rays" (n,) bool.  The mask is a pure function of per-ray data: shards
    reproduce it bit for bit.  The call synchronises once with the host (it reads the alive-ray count) and cannot be captured into a graph.
    ``camera`` (keyword-only; an addition): a ``nerf_amd.camera.Camera`` -- focal lengths, principal point and OpenCV / COLMAP lens distortion
    (include/nerf_amd.h) -- for a real capture: the ray table then comes from nerf_amd_generate_rays_camera, ``focal`` is IGNORED (pass
    anything), and ``ipe=True`` takes its pixel radius from ``camera.fx``.  Everything downstream of the ray table -- tiling, shards, every
    route and output -- is unchanged; ``Camera.reference(H, W, focal)`` renders the bits of the call without it.  The pose is the
    project's camera-to-world (3,4), looking down -z with y up: converting a COLMAP pose is the caller's job."""
    ops.ipe_contract(contract, ipe, ipe_cov, "nerf_amd.render_image")
    quantiles = ops.depth_quantiles(depth_quantiles, "nerf_amd.render_image")
    skip_dmin = ops.skip_threshold(skip_empty, None, "nerf_amd.render_image")
    render_opacity = bool(render_opacity)
    want_stats = bool(quantiles) or render_opacity
    if prop_rounds not in (1, 2):
        raise ValueError("nerf_amd.render_image: prop_rounds must be 1 or 2 (got %r)" % (prop_rounds,))
    if prop_pnum is not None and int(prop_pnum) < 1:
        raise ValueError("nerf_amd.render_image: prop_pnum must be positive")
    if prop_rounds == 2 and rng != "philox":
        raise ValueError("nerf_amd.render_image: prop_rounds=2 needs rng='philox' (the second round's uniforms are further columns of the ray's Philox stream)")
    if prop_rounds == 2 and type(network).__name__ == "RefNeRF":
        raise NotImplementedError("nerf_amd.render_image: the second proposal round is wired for the MipNeRF render path only")
    prop_pnum = RENDER_COARSE_PNUM if prop_pnum is None else int(prop_pnum)
    if not isinstance(image_size, Iterable):
        image_size = (image_size, image_size)
    is_ref_model = type(network).__name__ == "RefNeRF"
    render_normal = bool(render_normal) and is_ref_model
    H, W = int(image_size[0]), int(image_size[1])
    dev = render_pose.device
    if dev.type != "cuda":
        raise RuntimeError("nerf_amd.render_image: render_pose must live on the HIP device; there is no CPU path")
    if isinstance(focal, Iterable):
        fx, fy = float(focal[1]), float(focal[0])                                  # procedures.py:45-47
    else:
        fx = fy = float(focal)
    network._check_config()
    prop_net._check_config()
    prec = ops.current_precision()
    pose_rows = render_pose[:3]
    if getattr(render_pose, "_nerf_amd_host_pose", None) is not None:             # the pose's values, where its uploader kept them (metrics.evaluate_views):
        pose_rows._nerf_amd_host_pose = render_pose._nerf_amd_host_pose           # they ride on to the ray generator, which then reads nothing back
    if camera is not None:
        fx, fy = camera.fx, camera.fy
        rays = ops.generate_camera_rays(pose_rows, H, W, camera, dev)              # (H*W, 6), raster order
    else:
        rays = ops.generate_rays(pose_rows, H, W, fx, fy, dev)                     # (H*W, 6), raster order
    sz, patch_num = get_patch_size((H, W))
    if sz is not None:                                                             # reorder rays tile by tile
        pr, pc = patch_num
        rays = rays.view(H, W, 6)[: pr * sz].reshape(pr, sz, pc, sz, 6).permute(0, 2, 1, 3, 4).reshape(-1, 6).contiguous()
    if rng == "philox":
        u_strat = u_inv = None
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())                     # one draw from the CPU generator: torch.manual_seed governs it
    else:
        if _shard is not None:
            raise ValueError("nerf_amd.render_image: a ray shard needs rng='philox' (uniforms keyed by the global ray index)")
        seed = None
        u_strat, u_inv = _draw_uniforms(H, W, sample_num, sz, patch_num, dev, rng)
    off = 0
    # integrated PE: ONE direction norm over the call's rays (mip_methods.py:31) -- taken BEFORE a shard is cut out, so that every shard
    # encodes with the norm of the whole image and the gathered image equals the single-process one
    ipe_dir_norm = ops.dirs_norm(rays) if ipe else None
    if _shard is not None:
        off = int(_shard[0])
        rays = rays[off: int(_shard[1])].contiguous()
    z_base = _coarse_depths(near, far, dev)                                        # procedures.py:52 (CPU linspace bits)
    normal_px = None
    ipe_radius = None
    if ipe:
        if is_ref_model:
            raise NotImplementedError("nerf_amd: the integrated PE is wired for the MipNeRF render path only")
        ipe_radius = (2.0 / (12.0 ** 0.5) / fx) if ipe is True else float(ipe)
    generic = network._generic() or prop_net._generic()
    warped = _check_spacing(spacing, near, far)
    route = _render_route(is_ref_model, generic, warped, prop_rounds, prop_pnum)
    cam_dir = render_pose[:, -2].contiguous() if render_normal else None
    # depth quantiles / opacity: every route takes them as keywords and returns its dict last when either is set
    stat_kw = dict(quantiles=quantiles, want_opacity=render_opacity)
    if skip_dmin:
        stat_kw.update(skip_min_optical_depth=skip_dmin)
    if route == "calls":
        out = _render_rays_by_calls(network, prop_net, rays, z_base, u_strat, u_inv, sample_num, near, far, white_bkg, bool(render_depth),
                                    is_ref_model=is_ref_model, cam_dir=cam_dir, seed=seed, ray_offset=off, contract=contract,
                                    ipe_radius=ipe_radius, ipe_dir_norm=ipe_dir_norm, spacing=spacing, prop_rounds=prop_rounds,
                                    prop_pnum=prop_pnum, ipe_cov=ipe_cov, skip_min_optical_depth=skip_dmin or None, depth_quantiles=quantiles,
                                    render_opacity=render_opacity)
        rgb, depth, normal_px = out[:3]
    elif route == "ref":
        # procedures.py:71-74: coarse and fine depths are merged and sorted (a merge of two ascending sets), the last one dropped,
        # sigma -> softplus(sigma + 0.5) before compositing (nerf_amd_render_rays_ref: six launches)
        out = ops.render_rays_ref(prop_net.packed(prec), network.packed(prec), prec, rays, z_base, u_strat, u_inv, sample_num, near, far,
                                  white_bkg, want_depth=bool(render_depth), cam_dir=cam_dir, flags=network.kernel_flags, seed=seed,
                                  contract=contract, rng_ray_offset=off, **stat_kw)
        rgb, depth, normal_px = out[:3]
    else:
        # (a narrow fine network has no integrated-PE kernel: with ipe its 256-wide -- zero-padded -- blob is used)
        packed = (prop_net.packed(prec), network.packed(prec, wide=bool(ipe)), prec, rays)
        common = dict(want_depth=bool(render_depth), contract=ops.ipe_contract(contract, ipe, ipe_cov), ipe_radius=ipe_radius, ipe_dir_norm=ipe_dir_norm, seed=seed, rng_ray_offset=off,
                      **stat_kw)
        if route == "rounds":
            out = ops._render_rays_rounds(*packed, z_base, sample_num, near, far, white_bkg, prop_pnum=prop_pnum, spacing=spacing, **common)
        elif route == "warped":
            out = ops.render_rays_warped(*packed, u_strat, u_inv, sample_num, near, far, white_bkg, spacing=spacing, **common)
        else:
            out = ops.render_rays(*packed, z_base, u_strat, u_inv, sample_num, near, far, white_bkg, **common)
        rgb, depth = out[:2]
    stats = out[-1] if (want_stats or skip_dmin) else {"depth_q": None, "opacity": None}
    alive = stats["row_of_ray"] >= 0 if skip_dmin else None

    def to_image(t, ch):
        if sz is None:
            return t.view(H, W, ch).permute(2, 0, 1).contiguous()
        pr, pc = patch_num
        img = torch.zeros((ch, H, W), dtype=torch.float32, device=dev)
        img[:, : pr * sz] = t.view(pr, pc, sz, sz, ch).permute(4, 0, 2, 1, 3).reshape(ch, pr * sz, pc * sz)
        return img

    if _shard is not None:
        part = {"rgb_rays": rgb, "depth_rays": depth, "normal_rays": normal_px, "range": (off, off + rays.shape[0]), "to_image": to_image}
        if want_stats:
            part.update(depth_q_rays=stats["depth_q"], opacity_rays=stats["opacity"])
        if skip_dmin:
            part.update(alive_rays=alive)
        return part
    result = dict()
    result["rgb"] = to_image(rgb, 3)
    if render_depth:
        result["depth_img"] = to_image(depth.unsqueeze(-1), 1).expand(3, -1, -1).contiguous()   # procedures.py:88
    if render_normal:
        result["normal_img"] = to_image(normal_px.unsqueeze(-1), 1).expand(3, -1, -1).contiguous()   # procedures.py:90
    if quantiles:
        result["depth_quantiles"] = to_image(stats["depth_q"], len(quantiles))
    if render_opacity:
        result["opacity_img"] = to_image(stats["opacity"].unsqueeze(-1), 1)[0]
    if skip_dmin:
        result["alive_img"] = to_image(alive.to(torch.float32).unsqueeze(-1), 1)[0] > 0.5
        result["alive_fraction"] = stats["n_alive"] / (H * W)                   # of the image's pixels = alive_img.mean(); the host already has the count
    return result


def render_only(args, model_path: str, opt_level: str, dataset_root: str = "../dataset/", output_root: str = "./output/"):
    """Render-only entry point (procedures.py:99-164): load `<model_path><name>_{mip,prop}.pth`, render either the test-set poses
    (`-e`: with loss / PSNR against the ground truth) or a 120-view orbit `pose_spherical(angle, -30, 4)`, and write one PNG
    per view to `<output_root>{given,sphere}/result_%03d.png` (rgb [, depth, normal, ground truth] side by side).
    `opt_level` (apex) is accepted and ignored: `opt_mode == "native"` or `-s` select the bf16 kernels, anything else fp32.
    `dataset_root` / `output_root` default to the reference's hard-coded locations."""
    from tqdm import tqdm

    from .addtional import LossPSNR, SoftL1Loss
    from .dataset import AdaptiveResize, CustomDataSet, save_image, to_tensor
    from .utils import fov2Focal, pose_spherical
    resize = AdaptiveResize(args.img_scale)
    testset = CustomDataSet("%s%s/" % (dataset_root, args.dataset_name), lambda im: to_tensor(resize(im)), args.scene_scale, False, use_alpha=False)
    cam_fov_test, _ = testset.getCameraParam()
    r_c = testset.r_c()
    eval_poses = args.eval_poses
    render_normal = args.render_normal and not eval_poses
    render_depth = args.render_depth and not eval_poses
    if eval_poses:
        all_poses = testset.tfs.cuda()
        loss_func, psnr_func = SoftL1Loss(), LossPSNR()
    else:
        all_poses = torch.stack([pose_spherical(float(angle), -30.0, 4.0) for angle in torch.linspace(-180, 180, 120 + 1)[:-1]], 0).cuda()
    test_focal = fov2Focal(cam_fov_test, r_c)
    if args.ref_nerf:
        from .ref_model import RefNeRF
        mip_net = RefNeRF(10, args.ide_level, hidden_unit=args.nerf_net_width, perturb_bottle_neck_w=args.bottle_neck_noise, use_srgb=args.use_srgb).cuda()
    else:
        from .mip_model import MipNeRF
        mip_net = MipNeRF(10, 4, hidden_unit=args.nerf_net_width).cuda()
    prop_net = ProposalNetwork(10, hidden_unit=args.prop_net_width).cuda()
    mip_net.loadFromFile(model_path + args.name + "_mip.pth", False)
    prop_net.loadFromFile(model_path + args.name + "_prop.pth", False)
    mip_net.eval()
    prop_net.eval()
    low_precision = bool(args.use_scaler) or args.opt_mode == "native"
    eval_ssim = bool(eval_poses and getattr(args, "eval_ssim", False))            # an addition: off -> every line and PNG below is what it was
    if eval_ssim:
        from .metrics import image_metrics
        view_metrics = []
    with torch.no_grad():
        for i, pose in tqdm(list(enumerate(all_poses))):
            pose = pose.clone()
            pose[:3, -1] *= args.scene_scale
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=low_precision):
                result = render_image(mip_net, prop_net, pose[:3, :], r_c, test_focal, args.near, args.far, 128, white_bkg=args.white_bkg,
                                      render_normal=render_normal, render_depth=render_depth, skip_empty=getattr(args, "skip_empty", None))
            if eval_poses:
                gt_img = testset[i][0].cuda()
                loss = loss_func(result["rgb"], gt_img)
                print("Image loss:%.6f\tPSNR:%.4f" % (loss.item(), psnr_func(loss).item()))
                if eval_ssim:
                    m = image_metrics(result["rgb"].float().contiguous(), gt_img.float().contiguous())
                    view_metrics.append(torch.stack((m["psnr"][0], m["ssim"][0])))
                    print("Image SSIM:%.6f" % m["ssim"][0].item())
                result["gt_img"] = gt_img
            save_image(list(result.values()), "%s%s/result_%03d.png" % (output_root, "given" if eval_poses else "sphere", i),
                       nrow=1 + render_depth + render_depth + eval_poses)                  # (the reference counts render_depth twice)
    if eval_ssim and view_metrics:
        mean_psnr, mean_ssim = torch.stack(view_metrics).mean(0).tolist()          # means of the per-view values (the papers' convention)
        print("Test set (%d views): mean PSNR:%.4f\tmean SSIM:%.6f" % (len(view_metrics), mean_psnr, mean_ssim))
    mesh_path = getattr(args, "mesh", None)                                        # an addition: without it nothing above or below changes
    if mesh_path:
        from .mesh import extract_mesh, write_ply
        box = [float(v) for v in args.mesh_aabb]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=low_precision):
            mesh = extract_mesh(mip_net, (box[:3], box[3:]), args.mesh_res, args.mesh_iso, colors=True)
        write_ply(mesh_path, mesh["vertices"], mesh["faces"], mesh["normals"], mesh["colors"])
        print("Mesh: %d vertices, %d faces (iso %g, %d^3 lattice) -> %s" % (mesh["vertices"].shape[0], mesh["faces"].shape[0], args.mesh_iso, args.mesh_res, mesh_path))


def get_parser():
    """The reference's flag set (procedures.py:166-213) so that its entry scripts parse unchanged."""
    p = argparse.ArgumentParser()
    for name, typ, default, hlp in (
        ("--epochs", int, 2400, "Training lasts for . epochs"), ("--max_save", int, 3, "Check point max save number"),
        ("--sample_ray_num", int, 1024, "<x> rays to sample per training time"),
        ("--coarse_sample_pnum", int, 64, "Points to sample in coarse net"),
        ("--fine_sample_pnum", int, 128, "Points to sample in fine net"),
        ("--eval_time", int, 5, "Tensorboard output interval (train time)"),
        ("--output_time", int, 20, "Image output interval (train time)"),
        ("--center_crop_iter", int, 0, "Produce center"), ("--prop_net_width", int, 256, "Width of proposal network"),
        ("--nerf_net_width", int, 256, "Width of nerf network"), ("--near", float, 2., "Nearest sample depth"),
        ("--far", float, 6., "Farthest sample depth"), ("--center_crop_x", float, 0.5, "Center crop x axis ratio"),
        ("--center_crop_y", float, 0.5, "Center crop y axis ratio"), ("--name", str, "model_1", "Model name for loading"),
        ("--dataset_name", str, "lego", "Input dataset name in nerf synthetic dataset"),
        ("--img_scale", float, 0.5, "Scale of the image"), ("--scene_scale", float, 1.0, "Scale of the scene"),
        ("--grad_clip", float, -0.01, "Gradient clipping parameter (Negative number means no clipping)"),
        ("--pe_period_scale", float, 0.5, "Scale of positional encoding"),
        ("--opt_mode", str, "O1", "Optimization mode: none, native (torch amp), O1, O2 (apex amp)"),
        ("--min_ratio", float, 0.01, "Minimum for now_lr / lr"), ("--decay_rate", float, 0.1, "After <decay step>, lr = lr * <decay_rate>"),
        ("--decay_step", int, 100000, "After <decay step>, lr = lr * <decay_rate>"),
        ("--warmup_step", int, 500, "Warm up step (from lowest lr to starting lr)"), ("--lr", float, 1.5e-4, "Start lr"),
        ("--ide_level", int, 4, "Max level of spherical harmonics to be used"),
        ("--bottle_neck_noise", float, 0.02, "Noise std for perturbing bottle_neck vector"),
        ("--skip_empty", float, None, "(Render only; an addition) skip the fine network on rays whose proposal opacity is below this tau in (0, 1)"),
    ):
        p.add_argument(name, type=typ, default=default, help=hlp)
    for short, long_, hlp in (
        ("-d", "--del_dir", "Delete dir ./logs and start new tensorboard records"), ("-l", "--load", "Load checkpoint or trained model."),
        ("-s", "--use_scaler", "Use AMP scaler to speed up"), ("-b", "--debug", "Code debugging (detect gradient anomaly and NaNs)"),
        ("-v", "--visualize", "Visualize proposal network"), ("-r", "--do_render", "Only render the result"),
        ("-w", "--white_bkg", "Output white background"), ("-t", "--ref_nerf", "Test Ref NeRF"),
        ("-u", "--use_srgb", "Whether to use srgb in the output or not"), ("-e", "--eval_poses", "Whether to use test set poses to render image"),
    ):
        p.add_argument(short, long_, default=False, action="store_true", help=hlp)
    for long_, hlp in (("--render_depth", "Render depth image"), ("--render_normal", "Render normal image"),
                       ("--prop_normal", "(For proposal net) Whether to learn normals"),
                       ("--eval_ssim", "(Render only; an addition) with -e: print each view's SSIM too, and the test set's mean PSNR and mean SSIM")):
        p.add_argument(long_, default=False, action="store_true", help=hlp)
    # (Render only; additions) the density field's iso-surface as a PLY.  The defaults are conveniences for the Blender scenes, not measured choices.
    p.add_argument("--mesh", type=str, default=None, help="(Render only; an addition) also write the iso-surface of the fine network's density to this PLY file")
    p.add_argument("--mesh_res", type=int, default=256, help="Lattice points per axis of the mesh extraction")
    p.add_argument("--mesh_iso", type=float, default=10.0, help="Density level of the extracted surface")
    p.add_argument("--mesh_aabb", type=float, nargs=6, default=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], metavar=("x0", "y0", "z0", "x1", "y1", "z1"),
                   help="Box that the mesh lattice spans")
    return p
