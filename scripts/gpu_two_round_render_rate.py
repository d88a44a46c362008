#!/usr/bin/env python3
"""render_image at 800 x 800, 64 + 128 samples, prop_pnum = 64, bf16, timed with HIP events in one process: the one-round fused render
and the two-round render (`prop_rounds=2`), each under linear spacing (2, 6) and under disparity spacing (0.2, 1000) with contraction.
Uses only render_image's public keywords, so the same file times any tree that has `prop_rounds` -- the route a tree takes for two
rounds is that tree's own.  One JSON line on stdout and in `--out`.

    python scripts/gpu_two_round_render_rate.py --out profiles/two_round_render_rate.json
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
SPACINGS = {"linear": dict(near=2.0, far=6.0, kw=dict()), "disparity_contract": dict(near=0.2, far=1000.0, kw=dict(spacing="disparity", contract=True))}


def timed(fn, iters, warmup):
    """median / min / max ms of fn() over `iters` calls, one event pair per call"""
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    t = [ev[i].elapsed_time(ev[i + 1]) for i in range(iters)]
    return {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fine", type=int, default=128)
    ap.add_argument("--prop-pnum", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="one of: " + ", ".join(SPACINGS))
    ap.add_argument("--rounds", type=int, default=0, help="1 or 2: time only that many rounds (a kernel-trace run of one route); 0 = both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nerf_amd
    import weights                                             # tests/weights.py: the closed-form "small" parameter sets of the tests
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.procedures import render_image
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    nerf_amd.set_precision("bf16")
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.cuda().eval(), mip.cuda().eval()
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    res = {"fine": a.fine, "prop_pnum": a.prop_pnum, "iters": a.iters, "note": "ms per 800 x 800 render from HIP events; median, min, max; bf16"}
    with torch.no_grad():
        for name, s in SPACINGS.items():
            if a.only and a.only != name:
                continue
            out = {}
            for rounds in (1, 2):
                if a.rounds and a.rounds != rounds:
                    continue
                kw = dict(s["kw"], prop_rounds=2, prop_pnum=a.prop_pnum) if rounds == 2 else s["kw"]
                r = timed(lambda: render_image(mip, prop, pose, (H, W), focal, s["near"], s["far"], a.fine, seed=3, **kw), a.iters, a.warmup)
                r["rays_per_s"] = H * W / (r["ms"] * 1e-3)
                out["one_round" if rounds == 1 else "two_rounds"] = r
            if len(out) == 2:
                out["excess_ms"] = out["two_rounds"]["ms"] - out["one_round"]["ms"]
                out["two_over_one"] = out["two_rounds"]["ms"] / out["one_round"]["ms"]
            res[name] = out
            print(name, json.dumps(out), flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
