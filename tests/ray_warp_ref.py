"""The specification of the disparity ray spacing (Mip-NeRF 360's normalised distance s, Barron et al. 2022 section 3 / eq. 11-13 with
g(x) = 1/x), composed from the oracle's stage functions.  The reference has no such code: like the contraction this is the build's own
definition (include/nerf_amd.h), and these functions state it.  Everything here is plain torch on the CPU and runs
in whatever dtype its inputs have: fp32 reproduces the kernels' arithmetic step by step (torch rounds every operation on its own, like the
kernels built with -ffp-contract=off), fp64 is the yardstick.

    constants  gn = fp32(1/near), gf = fp32(1/far): computed in double, rounded once -- in EVERY dtype (they are part of the definition)
    warp       W(s)    = 1 / ((1 - sb) gn + sb gf),  sb = clamp(s, 0, 1)
    inverse    W^-1(z) = (1/zb - gn) / (gf - gn),    zb = clamp(z, near, far)
    coarse     s_j = (float)j r + u r,  r = fp32(1/C)
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nerf_oracle as O


def consts(near: float, far: float):
    """(gn, gf) as Python floats holding fp32 values"""
    if not 0.0 < near < far:
        raise ValueError("need 0 < near < far")
    return float(np.float32(1.0 / float(near))), float(np.float32(1.0 / float(far)))


def warp(s: torch.Tensor, near: float, far: float) -> torch.Tensor:
    gn, gf = consts(near, far)
    sb = s.clamp(0.0, 1.0)
    return 1.0 / ((1.0 - sb) * gn + sb * gf)


def unwarp(z: torch.Tensor, near: float, far: float) -> torch.Tensor:
    gn, gf = consts(near, far)
    lo, hi = float(np.float32(near)), float(np.float32(far))            # the kernels receive near / far as floats
    zb = z.clamp(lo, hi)
    if z.dtype == torch.float32:
        return (1.0 / zb - gn) / float(np.float32(gf) - np.float32(gn))
    return (1.0 / zb - gn) / (gf - gn)


def warp_np32(s: np.ndarray, near: float, far: float) -> np.ndarray:
    """W in numpy, every step an fp32 operation of its own"""
    f = np.float32
    gn, gf = (f(v) for v in consts(near, far))
    sb = np.minimum(np.maximum(s.astype(f), f(0)), f(1))
    a = (f(1) - sb) * gn
    b = sb * gf
    return f(1) / (a + b)


def unwarp_np32(z: np.ndarray, near: float, far: float) -> np.ndarray:
    f = np.float32
    gn, gf = (f(v) for v in consts(near, far))
    zb = np.minimum(np.maximum(z.astype(f), f(near)), f(far))
    return (f(1) / zb - gn) / (gf - gn)


def coarse_s(u: torch.Tensor) -> torch.Tensor:
    """u (N,C) -> s_c (N,C): the training sampler's expression at near = 0, res = fp32(1/C)"""
    C = u.shape[-1]
    r = float(np.float32(1.0) / np.float32(C))
    j = torch.arange(C, dtype=u.dtype)
    return j * r + u * r


def points(rays: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    return rays[:, None, :3] + rays[:, None, 3:] * z[:, :, None]


def proposal_weights(density: torch.Tensor, s_c: torch.Tensor, dirs: torch.Tensor, near: float, far: float, softplus: bool = False, alpha: float = 0.01):
    """weights from the METRIC depths W(s_c) |d| exactly as get_weights does, then maxBlurFilter"""
    dens = F.softplus(density) if softplus else density
    return O.max_blur(O.sigma_to_weights(dens, warp(s_c, near, far), dirs), alpha)


def resample(w_prop: torch.Tensor, s_c: torch.Tensor, u: torch.Tensor, near: float, far: float):
    """inverse sampling in s (bins = mid-points of s_c, pdf = w[1:-1] + 1e-5, sorted) -> (s_f, below, z_f = W(s_f))"""
    s_f, below = O.inverse_sample(w_prop, s_c, u, sort=True)
    return s_f, below, warp(s_f, near, far)


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def render_rays(prop_sd, mip_sd, rays, u_strat, u_inv, near, far, sample_num=128, white_bkg=False, contracted=False, dtype=torch.float32, stages=None,
                ipe_radius=None, ipe_dir_norm=None):
    """The non-Ref tile body under disparity spacing -> (rgb (N,3), weights (N,S), s-depth (N,) = W^-1(sum w z |d|)).  ``ipe_radius``: the
    fine network reads [mu | ipe_feature] of the frusta between the sample_num + 1 consecutive METRIC fine depths, as in oracle.render_rays"""
    prop_sd, mip_sd = _cast(prop_sd, dtype), _cast(mip_sd, dtype)
    rays, u_strat, u_inv = rays.to(dtype), u_strat.to(dtype), u_inv.to(dtype)
    s_c = coarse_s(u_strat)
    z_c = warp(s_c, near, far)
    pts_c = points(rays, z_c)
    density = O.proposal_forward(prop_sd, O.contract(pts_c) if contracted else pts_c)
    w_prop = proposal_weights(density, s_c, rays[:, 3:], near, far)
    s_f, below, z_all = resample(w_prop, s_c, u_inv, near, far)
    z_f = z_all[..., :-1]
    pts_f = O.length2pts(rays, z_f)
    enc = None
    if ipe_radius is not None:
        enc, mu, _ = O.ipe_feature(z_all, rays, 10, ipe_radius, ipe_dir_norm, contracted=contracted)      # (mu already contracted)
        pts_f = torch.cat((mu, pts_f[..., 3:]), dim=-1)
    elif contracted:
        pts_f = torch.cat((O.contract(pts_f[..., :3]), pts_f[..., 3:]), dim=-1)
    rgbo = O.mip_forward(mip_sd, pts_f, encoded_x=enc)
    rgb, w, extras = O.composite(rgbo, z_f, rays[:, 3:], white_bkg=white_bkg, render_depth=(0.0, 1.0))
    depth = unwarp(extras["depth_img"], near, far)
    if stages is not None:
        stages.update(s_coarse=s_c, z_coarse=z_c, density=density, w_prop=w_prop, s_fine=s_f, below=below, z_fine=z_all, rgbo=rgbo)
    return rgb, w, depth


def train_step(dtype, prop_sd, mip_sd, rays, s_c, s_all, below, tgt, near, far, contracted=True):
    """train.py:164-199 (non-ref) under disparity spacing on the oracle's expressions in `dtype`; the coarse and fine s and the bin indices
    are given (they carry no gradient) -> (image loss, proposal loss, rendered colours, {name: gradient})"""
    cast = lambda sd: {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    p, m = cast(prop_sd), cast(mip_sd)
    r = rays.to(dtype)
    zc, za = warp(s_c.to(dtype), near, far), warp(s_all.to(dtype), near, far)
    pts = points(r, zc)
    dens = F.softplus(O.proposal_forward(p, O.contract(pts) if contracted else pts))
    pw = O.max_blur(O.sigma_to_weights(dens, zc, r[:, 3:]), 0.01)
    zf = za[:, :-1]
    pts_f = O.length2pts(r, zf)
    if contracted:
        pts_f = torch.cat((O.contract(pts_f[..., :3]), pts_f[..., 3:]), -1)
    rgbo = O.mip_forward(m, pts_f)
    rend, wts, _ = O.composite(rgbo, zf, r[:, 3:])
    img = torch.mean((rend - tgt.to(dtype)) ** 2)
    ploss = O.proposal_loss(O.get_bounds(pw, below), wts.detach())
    (img + ploss).backward()
    grads = {"mip." + k: v.grad for k, v in m.items()}
    grads.update({"prop." + k: v.grad for k, v in p.items()})
    return img.item(), ploss.item(), rend.detach(), grads
