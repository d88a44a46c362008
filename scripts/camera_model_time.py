#!/usr/bin/env python3
"""What the camera model costs: (render) `render_image` 800 x 800 bf16 without a camera and with the strong OPENCV test camera, and the two
ray-table kernels alone; (sampler) the scene batch draw alone at 2^14 rays with and without per-view cameras, and the 2^14-ray MipNeRF
TrainStep (64 + 128 samples, bf16, learning rate 0) eager and replayed, with and without cameras, alternated in one process.

Timing as in scripts/scene_sampler_time.py (whose helpers this imports): windows of iterations between HIP events, a figure is the median
of the window medians with their range; a kernel alone is captured 50 times into one hipGraph so that the figure is device time.  With
NERF_AMD_LIB naming a library built from the parent commit only the camera-free arms run (the parent has no camera entry points): run
both libraries alternately for the parent-against-this-commit rows.

    python scripts/camera_model_time.py --out profiles/camera_model_time.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from scene_sampler_time import FAR, H, NEAR, W, figure, window      # noqa: E402


def nets(train):
    import weights
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.cuda(), mip.cuda()
    return (prop.train(), mip.train()) if train else (prop.eval(), mip.eval())


def captured_us(fn, reps=50, replays=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    ts, _ = window(lambda i: g.replay(), replays)
    return {"us": statistics.median(ts) / reps * 1e3, "min": min(ts) / reps * 1e3, "max": max(ts) / reps * 1e3}


def alternated(calls, a):
    for c in calls.values():
        for i in range(a.warmup):
            c(i)
    gpu = {k: [] for k in calls}
    for _ in range(a.repeats):
        for name, c in calls.items():
            g, _ = window(c, a.iters)
            gpu[name].append(statistics.median(g))
    return {k: figure(v) for k, v in gpu.items()}


def part_render(a, have_camera, pose, focal, camera):
    from nerf_amd.procedures import render_image
    from nerf_amd.utils import _focal_xy
    prop, mip = nets(False)
    fx, fy = _focal_xy(focal)
    out = {}
    with torch.no_grad():
        calls = {"no_camera": lambda i: render_image(mip, prop, pose, (H, W), focal, NEAR, FAR, 128, white_bkg=True, seed=7)}
        if have_camera:
            calls["opencv_camera"] = lambda i: render_image(mip, prop, pose, (H, W), focal, NEAR, FAR, 128, white_bkg=True, seed=7, camera=camera)
        out["render_image_ms"] = alternated(calls, argparse.Namespace(warmup=3, repeats=a.repeats, iters=a.render_iters))
        # (the pose is a device tensor: both wrappers read it back to the host per call, so the kernels are timed through the C entry points' launch alone)
        host = pose.cpu()
        rays = torch.empty((H * W, 6), dtype=torch.float32, device="cuda")
        import ctypes as C
        from nerf_amd._lib import lib
        p12 = (C.c_float * 12)(*host.reshape(-1).tolist()[:12])
        st = lambda: torch.cuda.current_stream().cuda_stream
        out["raygen_kernel_us"] = captured_us(lambda: lib.nerf_amd_generate_rays(p12, H, W, fx, fy, 0, H * W, rays.data_ptr(), st()))
        if have_camera:
            row = (C.c_float * 12)(*camera.row())
            out["raygen_camera_kernel_us"] = captured_us(lambda: lib.nerf_amd_generate_rays_camera(p12, H, W, row, 0, H * W, rays.data_ptr(), st()))
            ref = (C.c_float * 12)(*type(camera).reference(H, W, focal).row())
            out["raygen_camera_kernel_undistorted_us"] = captured_us(lambda: lib.nerf_amd_generate_rays_camera(p12, H, W, ref, 0, H * W, rays.data_ptr(), st()))
    return out


def part_sampler(a, have_camera, images, poses, focal, cameras):
    from nerf_amd import ops
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    from nerf_amd.utils import _focal_xy
    fx, fy = _focal_xy(focal)
    n = a.rays
    seed = torch.full((1,), 11, dtype=torch.int64, device="cuda")
    out = {"draw_us": {"no_cameras": captured_us(lambda: ops.sample_scene_rays(images, poses, fx, fy, NEAR, FAR, n, a.coarse, seed_dev=seed))}}
    if have_camera:
        out["draw_us"]["cameras"] = captured_us(lambda: ops.sample_scene_rays(images, poses, fx, fy, NEAR, FAR, n, a.coarse, seed_dev=seed, cameras=cameras))

    def step(**kw):
        prop, mip = nets(True)
        opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=0.0, lr_on_device=True)
        return TrainStep(prop, mip, opt, (H, W), focal, NEAR, FAR, ray_num=n, coarse_pnum=a.coarse, fine_pnum=a.fine, seed=11, scene=(images, poses), **kw)

    for graph in (False, True):
        steps = {"no_cameras": step()}
        if have_camera:
            steps["cameras"] = step(cameras=cameras)
        if graph:
            for s in steps.values():
                s.capture(warmup=3)
        out["step_%s_ms" % ("hipgraph" if graph else "eager")] = alternated({k: (lambda i, s=s: s()) for k, s in steps.items()}, a)
        assert all(bool(torch.isfinite(s.loss).item()) for s in steps.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["render", "sampler"])
    ap.add_argument("--rays", type=int, default=1 << 14)
    ap.add_argument("--coarse", type=int, default=64)
    ap.add_argument("--fine", type=int, default=128)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--render-iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("camera_model_time.py: needs a GPU (a CPU run measures nothing)")
    import nerf_amd
    from nerf_amd import _lib
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    import camera_ref as R
    nerf_amd.set_precision("bf16")
    have_camera = hasattr(_lib.lib, "nerf_amd_generate_rays_camera")
    focal = O.fov2focal(0.6911112070083618, (H, W))
    camera = R.camera_of(R.cameras(H, W)["opencv"])
    res = {"library": os.environ.get("NERF_AMD_LIB") or "this tree", "camera_entry_points": have_camera, "camera_row": camera.row()}
    if "render" in a.parts:
        res["render"] = part_render(a, have_camera, O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda(), focal, camera)
    if "sampler" in a.parts:
        gen = torch.Generator(device="cuda").manual_seed(0)
        images = torch.rand((a.views, 3, H, W), generator=gen, device="cuda")
        poses = torch.stack([O.pose_spherical(3.6 * v, -30.0, 4.0)[:3] for v in range(a.views)]).contiguous().cuda()
        cams = [R.camera_of(R.cameras(H, W)[("opencv", "simple_radial", "pinhole")[v % 3]]) for v in range(a.views)]
        res["sampler"] = part_sampler(a, have_camera, images, poses, focal, type(camera).table(cams, "cuda") if have_camera else None)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
