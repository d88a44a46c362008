#!/usr/bin/env python3
"""Cost of ipe_cov="contracted" (the frustum covariance pushed through the scene contraction) against ipe_cov="metric", both in ONE process
on the same device:

  * render_image at 800 x 800, 64 + 128 samples, bf16, ipe=True, contract=True, in-kernel Philox uniforms: the settings ALTERNATED,
    `--iters` timed images each (HIP events around each call);
  * the 2^14-ray scene-mode TrainStep (4 views of 800 x 800, 64 + 128, bf16, same flags, learning rate 0 so that both settings time the
    same network state), eager, alternated in blocks of `--block` steps.

`--settings metric` times the default alone: with NERF_AMD_LIB pointing at a library built from the parent commit (nerf_amd/_lib.py: a
diagnostic build of an older tree) the same script gives the parent's figure for the unchanged arithmetic -- run the two libraries in
alternating processes.  A library without nerf_amd_ipe_feature_gaussian is refused "contracted".  Writes one JSON to `--out` (median,
mean, standard deviation, min, max in ms per setting).

    python scripts/gpu_ipe_cov_rate.py --out profiles/ipe_cov_rate.json
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
H = W = 800
NEAR, FAR = 0.2, 30.0


def nets(train):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    import weights                                             # tests/weights.py: the closed-form "small" parameter sets of the tests
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.cuda(), mip.cuda()
    return (prop.train(), mip.train()) if train else (prop.eval(), mip.eval())


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "sd_ms": statistics.pstdev(ms), "min_ms": min(ms), "max_ms": max(ms),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="timed images / steps per setting")
    ap.add_argument("--block", type=int, default=5, help="training steps per alternation block")
    ap.add_argument("--rays", type=int, default=1 << 14)
    ap.add_argument("--settings", default="metric,contracted")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nerf_amd
    from nerf_amd import _lib
    from nerf_amd.optim import Adam
    from nerf_amd.procedures import render_image
    from nerf_amd.training import TrainStep
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    settings = a.settings.split(",")
    if "contracted" in settings and not hasattr(_lib.lib, "nerf_amd_ipe_feature_gaussian"):
        sys.exit("this library has no contracted-covariance mode: --settings metric")
    nerf_amd.set_precision("bf16")
    pose = O.pose_spherical(30.0, -30.0, 1.5)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    out = {"library": os.environ.get("NERF_AMD_LIB") or "in-tree",
           "shape": {"H": H, "W": W, "coarse": 64, "fine": 128, "near": NEAR, "far": FAR, "precision": "bf16", "contract": True, "ipe": True}}

    prop, mip = nets(False)
    render = {s: [] for s in settings}
    with torch.no_grad():
        def one(cov):
            return render_image(mip, prop, pose, (H, W), focal, NEAR, FAR, 128, white_bkg=True, contract=True, ipe=True, seed=7, ipe_cov=cov)
        for cov in render:                                     # warm-up: lazy kernel loads, packed blobs, allocator pools
            for _ in range(2):
                one(cov)
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for cov in render:
                render[cov].append(timed(lambda: one(cov)))
    out["render_image_800x800"] = {k: stats(v) for k, v in render.items()}

    images = torch.rand(4, 3, H, W, device="cuda")
    poses = torch.stack([O.pose_spherical(20.0 + 40.0 * v, -25.0, 1.5)[:3] for v in range(4)]).contiguous().cuda()
    from nerf_amd.utils import _focal_xy
    radius = 2.0 / 12.0 ** 0.5 / _focal_xy(focal)[0]           # render_image's ipe=True
    steps, train = {}, {s: [] for s in settings}
    for cov in train:
        p, m = nets(True)
        opt = Adam(list(m.parameters()) + list(p.parameters()), lr=0.0, lr_on_device=True)
        steps[cov] = TrainStep(p, m, opt, (H, W), focal, NEAR, FAR, ray_num=a.rays, coarse_pnum=64, fine_pnum=128, seed=11, contract=True,
                               ipe_radius=radius, scene=(images, poses), ipe_cov=cov)
        for _ in range(3):
            steps[cov]()
    torch.cuda.synchronize()
    done = 0
    while done < a.iters:
        for cov in train:
            for _ in range(a.block):
                train[cov].append(timed(steps[cov]))
        done += a.block
    out["scene_train_step_%d_rays" % a.rays] = {k: stats(v) for k, v in train.items()}
    if len(settings) == 2:
        for name, d in out.items():
            if name not in ("shape", "library"):
                d["contracted_over_metric_median"] = d["contracted"]["median_ms"] / d["metric"]["median_ms"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
