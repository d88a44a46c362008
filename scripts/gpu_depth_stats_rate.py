#!/usr/bin/env python3
"""What depth quantiles and opacity cost on an MI355X (profiles/depth_stats_summary.md):

  * render_image 800 x 800, bf16, 128 fine samples, with and without depth_quantiles=(0.5,), render_opacity=True, alternated in one
    process, under linear spacing and under disparity spacing with contraction;
  * the stats kernel alone on (640 000, 128) weights and closed depth rows, device events around batches of launches.

    python scripts/gpu_depth_stats_rate.py [--reps 12] [--side 800]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--side", type=int, default=800)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    import nerf_amd
    from nerf_amd import ops, procedures, synthetic_weights as W
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from oracle import nerf_oracle as O
    nerf_amd.set_precision("bf16")
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small"))
    prop, mip = prop.cuda().eval(), mip.cuda().eval()
    side = args.side
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (side, side))
    for name, near, far, kw in (("linear", 2.0, 6.0, dict()), ("disparity + contract", 0.2, 100.0, dict(spacing="disparity", contract=True))):
        def render(extras):
            with torch.no_grad():
                procedures.render_image(mip, prop, pose, side, focal, near, far, 128, white_bkg=True, render_depth=True, seed=7,
                                        **(dict(depth_quantiles=(0.5,), render_opacity=True) if extras else dict()), **kw)
        for extras in (False, True):
            timed(lambda: render(extras), 3)                                                # warm-up of both variants
        off, on = [], []
        for _ in range(args.reps):                                                          # alternated: A B A B ...
            off += timed(lambda: render(False), 1)
            on += timed(lambda: render(True), 1)
        print("render_image %dx%d bf16 %-22s without %.3f ms (min %.3f max %.3f)  with %.3f ms (min %.3f max %.3f)  median difference %.3f ms"
              % (side, side, name, statistics.median(off), min(off), max(off), statistics.median(on), min(on), max(on),
                 statistics.median(on) - statistics.median(off)), flush=True)
    N, S = side * side, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.rand((N, S), device="cuda", generator=g)
    w = w / w.sum(-1, keepdim=True) * 0.9
    z = torch.sort(2.0 + 4.0 * torch.rand((N, S + 1), device="cuda", generator=g), dim=-1)[0].contiguous()
    rays = torch.randn((N, 6), device="cuda", generator=g)
    for qs in ((0.5,), (0.1, 0.25, 0.5, 0.9)):
        for _ in range(5):
            ops.ray_depth_stats(w, z, rays, quantiles=qs)
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                ops.ray_depth_stats(w, z, rays, quantiles=qs)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b) / 10)
        nbytes = N * (S * 4 + (S + 1) * 4 + 12 + 4 + 4 * len(qs))
        med = statistics.median(times)
        print("ray_depth_stats (%d, %d), %d quantile(s) + opacity: %.4f ms per launch (min %.4f max %.4f; includes the op's two allocations), %.2f GB moved, %.2f TB/s"
              % (N, S, len(qs), med, min(times), max(times), nbytes / 1e9, nbytes / med / 1e9), flush=True)


if __name__ == "__main__":
    main()
