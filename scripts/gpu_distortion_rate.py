#!/usr/bin/env python3
"""Cost of TrainStep(distortion=...) (Mip-NeRF 360's L_dist on the fine weights, nerf_amd_distortion_loss[_backward]): the MipNeRF step at
2^14 rays, 64 + 128 samples, plain and contract=True, eager and replayed from a hipGraph, with distortion 0 and 0.01 ALTERNATED in one
process from the same parameters (tests/weights.py "small", learning rate 0; blocks of `--block` steps each, `--iters` timed steps per setting), timed with HIP events.  Writes one JSON to `--out`.
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats (`--iters 30 --block 30` keeps that run short).

    python scripts/gpu_distortion_rate.py --out profiles/distortion_rate.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
H = W = 800


def make_step(lam, contract, graph, img, pose, focal, n_rays, c_n, f_n):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    import weights                                             # tests/weights.py: the closed-form "small" parameter sets of the tests
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.cuda().train(), mip.cuda().train()
    # lr 0: the Adam launch runs, the parameters stay put -- both settings time the same network state (a training run from torch's
    # default init can zero every density within a few steps, and data-dependent sampling work would then differ between the two)
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=0.0, lr_on_device=True)
    near, far = (0.2, 12.0) if contract else (2.0, 6.0)
    st = TrainStep(prop, mip, opt, (H, W), focal, near, far, ray_num=n_rays, coarse_pnum=c_n, fine_pnum=f_n, seed=11, contract=contract,
                   distortion=lam)
    st.set_image(img, pose)
    if graph:
        st.capture(warmup=3)
    for _ in range(3):
        st()
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 14)
    ap.add_argument("--coarse", type=int, default=64)
    ap.add_argument("--fine", type=int, default=128)
    ap.add_argument("--iters", type=int, default=60, help="timed steps per setting")
    ap.add_argument("--block", type=int, default=10, help="steps per alternation block")
    ap.add_argument("--lam", type=float, default=0.01)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nerf_amd
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    nerf_amd.set_precision("bf16")
    img = torch.rand(3, H, W, device="cuda")
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    res = {"rays": a.rays, "coarse": a.coarse, "fine": a.fine, "lambda": a.lam, "iters_per_setting": a.iters, "block": a.block,
           "pairs_per_step": a.rays * a.fine * a.fine, "note": "ms per TrainStep iteration from HIP events, settings alternated in blocks"}
    for contract in (False, True):
        for graph in (False, True):
            key = "%s_%s" % ("contract" if contract else "plain", "hipgraph" if graph else "eager")
            steps = {lam: make_step(lam, contract, graph, img, pose, focal, a.rays, a.coarse, a.fine) for lam in (0.0, a.lam)}
            times = {0.0: [], a.lam: []}
            while len(times[a.lam]) < a.iters:
                for lam, st in steps.items():
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.block + 1)]
                    ev[0].record()
                    for i in range(a.block):
                        st()
                        ev[i + 1].record()
                    torch.cuda.synchronize()
                    times[lam] += [ev[i].elapsed_time(ev[i + 1]) for i in range(a.block)]
            med0, med1 = statistics.median(times[0.0]), statistics.median(times[a.lam])
            res[key] = {"ms_distortion_0": med0, "ms_distortion_on": med1, "added_ms": med1 - med0, "added_pct": 100.0 * (med1 - med0) / med0,
                        "spread_ms_distortion_0": [min(times[0.0]), max(times[0.0])], "spread_ms_distortion_on": [min(times[a.lam]), max(times[a.lam])],
                        "dist_loss": float(steps[a.lam].dist_loss.item()), "loss_finite": bool(torch.isfinite(steps[a.lam].loss).item())}
            print(key, json.dumps(res[key]), flush=True)
            del steps
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
