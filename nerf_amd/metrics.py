"""Image quality on the device: PSNR and SSIM of rendered views against their ground truth (nerf_amd_image_metrics, include/nerf_amd.h),
and the test-set table built from them.  An addition of this build: the reference compares one image with its ground truth through
``SoftL1Loss`` -> ``LossPSNR`` and has no SSIM.

Definition.  Images are fp32 (V, C, H, W) -- (C, H, W) is one view --, nominally in [0, 1], dynamic range L = 1.
  mse[v]   the mean of (pred - target)^2 over all C H W elements: what ``SoftL1Loss`` computes per image.
  psnr[v]  -10 log10(mse[v]) in fp64, +inf for identical images like ``LossPSNR`` on 0.  This is the EXACT ln 10: ``LossPSNR`` multiplies
           an fp32 log by an fp32-rounded constant -10 / ln 10, a relative difference of about 1e-8.
  ssim[v]  Wang et al.'s SSIM with the 11 x 11 Gaussian window (sigma 1.5, separable, normalised), C1 = 0.01^2, C2 = 0.03^2, evaluated at
           VALID positions only -- (H - 10) x (W - 10) per channel, no padding -- and averaged over channels and positions.
All three are fp64 device tensors of shape (V,); nothing is read back to the host."""
from typing import Optional

import torch

from . import ops

__all__ = ["image_metrics", "SSIM", "PSNR", "evaluate_views"]


def _forward_only(who: str, *tensors):
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise RuntimeError("%s is forward only: there is no backward kernel, and it will not return a wrong gradient -- call it under "
                           "torch.no_grad() or on detached tensors" % who)


def image_metrics(pred: torch.Tensor, target: torch.Tensor, *, want_map: bool = False) -> dict:
    """{"mse", "psnr", "ssim"} -- (V,) fp64 device tensors, see the module's docstring -- and, with ``want_map``, "ssim_map"
    (V, C, H - 10, W - 10) fp32, the SSIM of every valid position (error maps).  ``pred`` and ``target``: contiguous fp32 device tensors
    of one shape, H, W >= 11 (``ValueError`` otherwise, before anything is launched).  Forward only."""
    _forward_only("nerf_amd.metrics.image_metrics", pred, target)
    with torch.no_grad():
        out = ops.image_metrics(pred, target, want_map=want_map)
        result = {"mse": out[0], "psnr": -10.0 * torch.log10(out[0]), "ssim": out[1]}
        if want_map:
            result["ssim_map"] = out[2]
    return result


class SSIM(torch.nn.Module):
    """forward(pred, target) -> (V,) fp64 SSIM per view (``image_metrics``).  Forward only: inputs that require grad raise."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return image_metrics(pred, target)["ssim"]


class PSNR(torch.nn.Module):
    """forward(pred, target) -> (V,) fp64 PSNR per view in dB (``image_metrics``; the exact ln 10, see the module's docstring).  Forward
    only: inputs that require grad raise."""

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return image_metrics(pred, target)["psnr"]


def evaluate_views(network, prop_net, images: torch.Tensor, poses, focal, near: float, far: float, *, sample_num: int = 128, white_bkg: bool = False,
                   seed: Optional[int] = None, camera=None, **render_kw) -> dict:
    """Render the V ``poses`` with ``procedures.render_image`` at the size of ``images`` (V, 3, H, W), the ground truth, and compare:
    {"psnr", "ssim", "mse"} per view, (V,) fp64, and "mean_psnr", "mean_ssim", the means of the PER-VIEW values (the papers' convention:
    the mean PSNR is not the PSNR of the mean error), 0-d fp64 -- all device tensors.  Every view is written into one (V, 3, H, W) buffer
    and the metric runs once for all of them.  ``seed``: view v renders with ``seed + v`` (None: render_image's own draw per view).
    ``camera``: one ``nerf_amd.camera.Camera`` for all views, or a sequence of V.  ``render_kw`` goes to render_image as it is and keeps
    its own behaviour there (``skip_empty``, for one, still reads its ray count).  ``poses``: (V, 3 or 4, 4), camera-to-world.  Give them
    as a HOST tensor: this function uploads them once (pinned, asynchronous) and hands render_image their host values along with the
    device rows, so that the whole call -- with rng="philox" and a seed -- neither reads the device nor waits for it, and the test set is
    evaluated without one host synchronisation (the coarse depths are uploaded by the first render of a (near, far) pair in the
    process).  Device poses work too; render_image then reads each one back, as it always has.  The caller provides ``no_grad`` /
    ``eval()`` and autocast like for render_image."""
    from .procedures import render_image
    for name in ("render_pose", "image_size", "_shard"):
        if name in render_kw:
            raise ValueError("nerf_amd.metrics.evaluate_views: '%s' is not a keyword of this call" % name)
    V, C_, H, W = ops._image_metrics_args(images, images, "nerf_amd.metrics.evaluate_views")
    if images.dim() != 4 or C_ != 3:
        raise ValueError("nerf_amd.metrics.evaluate_views: images must be (V, 3, H, W) (got %s)" % (tuple(images.shape),))
    if len(poses) != V:
        raise ValueError("nerf_amd.metrics.evaluate_views: %d poses for %d images" % (len(poses), V))
    per_view_camera = camera is not None and isinstance(camera, (list, tuple))
    if per_view_camera and len(camera) != V:
        raise ValueError("nerf_amd.metrics.evaluate_views: %d cameras for %d images" % (len(camera), V))
    if not isinstance(poses, torch.Tensor):
        poses = torch.stack([torch.as_tensor(p) for p in poses])
    if poses.dim() != 3 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
        raise ValueError("nerf_amd.metrics.evaluate_views: poses must be (V, 3, 4) or (V, 4, 4) (got %s)" % (tuple(poses.shape),))
    host_rows = None
    if not poses.is_cuda:
        staged = poses.detach().to(torch.float32)[:, :3].contiguous()
        host_rows = staged.reshape(V, 12).tolist()
        poses = staged.pin_memory().to(images.device, non_blocking=True)
    pred = torch.empty((V, 3, H, W), dtype=torch.float32, device=images.device)
    for v in range(V):
        pose = poses[v][:3]
        if host_rows is not None:
            pose._nerf_amd_host_pose = host_rows[v]                                 # rides on the tensor object: render_image does not read it back
        out = render_image(network, prop_net, pose, (H, W), focal, near, far, sample_num, white_bkg=white_bkg,
                           seed=None if seed is None else int(seed) + v, camera=camera[v] if per_view_camera else camera, **render_kw)
        pred[v].copy_(out["rgb"])
    result = image_metrics(pred, images)
    result["mean_psnr"] = result["psnr"].mean()
    result["mean_ssim"] = result["ssim"].mean()
    return result
