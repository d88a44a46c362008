#!/usr/bin/env python3
"""Cost of spacing="disparity" against spacing="linear", both in ONE process on the same device:

  * render_image at 800 x 800, 64 + 128 samples, bf16, contract=True, in-kernel Philox uniforms: the two spacings ALTERNATED, `--iters`
    timed images each (HIP events around each call);
  * the 2^14-ray scene-mode TrainStep (4 views of 800 x 800, 64 + 128, bf16, contract=True, learning rate 0 so that both settings time the
    same network state), eager, alternated in blocks of `--block` steps.

Near / far are (0.2, 30) for both spacings: the numbers compare the code paths on the same scene, not two scenes.  Writes one JSON to
`--out` (median, mean, standard deviation, min, max in ms per setting).

    python scripts/gpu_ray_warp_rate.py --out profiles/ray_warp_rate.json
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nerf_amd
    from nerf_amd.optim import Adam
    from nerf_amd.procedures import render_image
    from nerf_amd.training import TrainStep
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    nerf_amd.set_precision("bf16")
    pose = O.pose_spherical(30.0, -30.0, 1.5)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    out = {"shape": {"H": H, "W": W, "coarse": 64, "fine": 128, "near": NEAR, "far": FAR, "precision": "bf16", "contract": True}}

    prop, mip = nets(False)
    render = {"linear": [], "disparity": []}
    with torch.no_grad():
        def one(sp):
            return render_image(mip, prop, pose, (H, W), focal, NEAR, FAR, 128, white_bkg=True, contract=True, seed=7, spacing=sp)
        for sp in render:                                      # warm-up: lazy kernel loads, packed blobs, allocator pools
            for _ in range(2):
                one(sp)
        torch.cuda.synchronize()
        for _ in range(a.iters):
            for sp in render:
                render[sp].append(timed(lambda: one(sp)))
    out["render_image_800x800"] = {k: stats(v) for k, v in render.items()}

    images = torch.rand(4, 3, H, W, device="cuda")
    poses = torch.stack([O.pose_spherical(20.0 + 40.0 * v, -25.0, 1.5)[:3] for v in range(4)]).contiguous().cuda()
    steps, train = {}, {"linear": [], "disparity": []}
    for sp in train:
        p, m = nets(True)
        opt = Adam(list(m.parameters()) + list(p.parameters()), lr=0.0, lr_on_device=True)
        steps[sp] = TrainStep(p, m, opt, (H, W), focal, NEAR, FAR, ray_num=a.rays, coarse_pnum=64, fine_pnum=128, seed=11, contract=True,
                              scene=(images, poses), spacing=sp)
        for _ in range(3):
            steps[sp]()
    torch.cuda.synchronize()
    done = 0
    while done < a.iters:
        for sp in train:
            for _ in range(a.block):
                train[sp].append(timed(steps[sp]))
        done += a.block
    out["scene_train_step_%d_rays" % a.rays] = {k: stats(v) for k, v in train.items()}
    for name, d in out.items():
        if name != "shape":
            d["disparity_over_linear_median"] = d["disparity"]["median_ms"] / d["linear"]["median_ms"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
