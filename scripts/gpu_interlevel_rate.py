#!/usr/bin/env python3
"""Cost of the interlevel loss and of the second proposal round, all in one process on one box, timed with HIP events:

  kernels  nerf_amd_interlevel_loss + _backward alone at N = 2^14, M = 128, K = 64 (open form) against the ops they replace,
           getBounds + ProposalLoss forward and backward (HIP get_bounds[_backward] + the torch expression of ProposalLoss);
  step     the 2^14-ray MipNeRF TrainStep, 64 + 128 samples, in four variants -- reference loss; interlevel, one round; interlevel,
           two rounds; two rounds with contract + spacing="disparity" + distortion -- each eager and replayed from a hipGraph, from the
           same parameters (tests/weights.py "small", learning rate 0), the variants ALTERNATED in blocks of `--block` steps;
  render   render_image at 800 x 800, bf16: the fused one-round route against the call-by-call two-round route.

Writes one JSON to `--out`.

    python scripts/gpu_interlevel_rate.py --out profiles/interlevel_rate.json
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
VARIANTS = {
    "reference": dict(),
    "interlevel_1": dict(prop_loss="interlevel"),
    "interlevel_2": dict(prop_loss="interlevel", prop_rounds=2),
    "interlevel_2_contract_disparity_distortion": dict(prop_loss="interlevel", prop_rounds=2, contract=True, spacing="disparity", distortion=0.01),
}


def timed(fn, iters, warmup=5):
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


def nets(train):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    import weights                                             # tests/weights.py: the closed-form "small" parameter sets of the tests
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    return (prop.cuda().train(), mip.cuda().train()) if train else (prop.cuda().eval(), mip.cuda().eval())


def kernels(a):
    import interlevel_ref as R                                 # tests/interlevel_ref.py: the tests' input generator
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalLoss, getBounds
    N, M, K = a.rays, a.fine, a.coarse
    w, t, w_prop, t_prop = (x.cuda() for x in R.make_inputs(N, M, K, True, False, 1))
    g = torch.ones((), device="cuda")
    below = torch.searchsorted(t_prop.contiguous(), t.contiguous(), right=True).clamp(1, K - 1)      # bin indices like the sampler's
    p = w_prop.clone().requires_grad_(True)

    def reference():
        p.grad = None
        ProposalLoss()(getBounds(p, below), w).backward()

    res = {"N": N, "M": M, "K": K,
           "interlevel_forward": timed(lambda: ops.interlevel_loss(w, t, w_prop, t_prop, 1.0), a.iters),
           "interlevel_backward": timed(lambda: ops.interlevel_loss_backward(g, w, t, w_prop, t_prop, 1.0), a.iters),
           "interlevel_forward_with_bounds": timed(lambda: ops.interlevel_loss(w, t, w_prop, t_prop, 1.0, want_bounds=True), a.iters),
           "getbounds_proposalloss_forward_backward": timed(reference, a.iters)}
    res["interlevel_forward_backward_ms"] = res["interlevel_forward"]["ms"] + res["interlevel_backward"]["ms"]
    return res


def make_step(kw, graph, img, pose, focal, a):
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    prop, mip = nets(True)
    # lr 0: the Adam launch runs, the parameters stay put -- every variant times the same network state
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=0.0, lr_on_device=True)
    near, far = (0.2, 12.0) if kw.get("contract") else (2.0, 6.0)
    st = TrainStep(prop, mip, opt, (H, W), focal, near, far, ray_num=a.rays, coarse_pnum=a.coarse, fine_pnum=a.fine, seed=11, **kw)
    st.set_image(img, pose)
    if graph:
        st.capture(warmup=3)
    for _ in range(3):
        st()
    return st


def steps(a, img, pose, focal):
    res = {}
    for graph in (False, True):
        sts = {name: make_step(kw, graph, img, pose, focal, a) for name, kw in VARIANTS.items()}
        times = {name: [] for name in sts}
        while len(times["reference"]) < a.iters:
            for name, st in sts.items():
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.block + 1)]
                ev[0].record()
                for i in range(a.block):
                    st()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                times[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(a.block)]
        for name, st in sts.items():
            key = "%s_%s" % (name, "hipgraph" if graph else "eager")
            res[key] = {"ms": statistics.median(times[name]), "min_ms": min(times[name]), "max_ms": max(times[name]),
                        "prop_loss_value": float(st.prop_loss_value.item()), "loss_finite": bool(torch.isfinite(st.loss).item())}
            print(key, json.dumps(res[key]), flush=True)
        del sts
        torch.cuda.empty_cache()
    return res


def render(a, pose, focal):
    from nerf_amd.procedures import render_image
    prop, mip = nets(False)
    res = {}
    with torch.no_grad():
        for name, kw in (("fused_one_round", dict()), ("by_calls_two_rounds", dict(prop_rounds=2))):
            r = timed(lambda: render_image(mip, prop, pose, (H, W), focal, 2.0, 6.0, a.fine, seed=3, **kw), a.render_iters, warmup=2)
            r["rays_per_s"] = H * W / (r["ms"] * 1e-3)
            res[name] = r
            print("render", name, json.dumps(r), flush=True)
    res["two_rounds_over_fused"] = res["by_calls_two_rounds"]["ms"] / res["fused_one_round"]["ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 14)
    ap.add_argument("--coarse", type=int, default=64)
    ap.add_argument("--fine", type=int, default=128)
    ap.add_argument("--iters", type=int, default=60, help="timed calls / steps per setting")
    ap.add_argument("--block", type=int, default=10, help="steps per alternation block")
    ap.add_argument("--render-iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import nerf_amd
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    nerf_amd.set_precision("bf16")
    img = torch.rand(3, H, W, device="cuda")
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    res = {"rays": a.rays, "coarse": a.coarse, "fine": a.fine, "iters_per_setting": a.iters, "block": a.block,
           "note": "ms from HIP events; step variants alternated in blocks; bf16"}
    res["kernels"] = kernels(a)
    print("kernels", json.dumps(res["kernels"]), flush=True)
    res["step"] = steps(a, img, pose, focal)
    res["render"] = render(a, pose, focal)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
