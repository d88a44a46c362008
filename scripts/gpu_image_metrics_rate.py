#!/usr/bin/env python3
"""Cost of nerf_amd_image_metrics (SSIM + MSE per view) and of metrics.evaluate_views, on the GPU, timed with HIP events.

  kernels   ops.image_metrics at (1, 3, 800, 800) and at (200, 3, 800, 800), the Lego test set, ALTERNATED in one process with a plain
            torch-on-device SSIM of the same definition written here (five grouped conv2d per pass, separable, valid, fp32; its means by
            torch.mean) -- the thing a user would write by hand.  The traffic floor is two reads of the inputs (8 bytes per element) at
            the HBM rate DESIGN.md measured on these boxes (--hbm-tbs, 5 TB/s); the achieved GB/s is the same bytes over the measured time.
  views     evaluate_views per view against render_image alone (same networks: the closed-form "small" weights, bf16, 128 fine samples),
            alternated, with the min-max spread.
Writes one JSON to `--out`.

    python scripts/gpu_image_metrics_rate.py --out profiles/image_metrics_rate.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_ssim_mse(pred, target, g):
    """the definition in plain torch on the device: (mse (V,), ssim (V,)) fp32"""
    import torch.nn.functional as F
    V, C, H, W = pred.shape
    x, y = pred.reshape(V * C, 1, H, W), target.reshape(V * C, 1, H, W)
    kh, kv = g.view(1, 1, 1, 11), g.view(1, 1, 11, 1)
    blur = lambda t: F.conv2d(F.conv2d(t, kh), kv)
    mx, my = blur(x), blur(y)
    vx, vy, cxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    s = (2 * mx * my + 1e-4) * (2 * cxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    return ((pred - target) ** 2).reshape(V, -1).mean(1), s.reshape(V, -1).mean(1)


def time_ms(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(fns, iters, blocks):
    """{name: [ms per call of each block]}: the candidates take turns, block by block"""
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            out[k].append(time_ms(fn, iters))
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "blocks": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--hbm-tbs", type=float, default=5.0, help="HBM rate of the traffic floor, TB/s")
    ap.add_argument("--render-views", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to measure without one"
    import nerf_amd
    from nerf_amd import metrics, ops, procedures
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import image_metrics_ref as R
    g = torch.from_numpy(R.window32()).cuda()
    result = {"device": torch.cuda.get_device_name(0), "hbm_tbs_assumed": a.hbm_tbs, "kernels": {}}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for V in (1, a.views):
        shape = (V, 3, a.size, a.size)
        target = torch.rand(shape, device="cuda", generator=gen)
        pred = (target + 0.1 * torch.randn(shape, device="cuda", generator=gen)).clamp_(0, 1)
        ours = lambda: ops.image_metrics(pred, target)
        ours_map = lambda: ops.image_metrics(pred, target, want_map=True)
        plain = lambda: torch_ssim_mse(pred, target, g)
        m_o, s_o = ours()
        m_t, s_t = plain()
        agree = {"ssim_max_abs_diff": float((s_o - s_t.double()).abs().max()), "mse_max_rel_diff": float(((m_o - m_t.double()) / m_o).abs().max())}
        for fn in (ours, ours_map, plain):                                       # warm every candidate at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = 200 if V == 1 else 5
        t = alternate({"image_metrics": ours, "image_metrics_with_map": ours_map, "torch_conv2d": plain}, iters, a.blocks)
        nbytes = 2 * 4 * pred.numel()
        floor_ms = nbytes / (a.hbm_tbs * 1e12) * 1e3
        row = {k: summary(v) for k, v in t.items()}
        for k in row:
            row[k]["input_gb_per_s"] = nbytes / (row[k]["median_ms"] * 1e-3) / 1e9
        row.update(shape=list(shape), input_bytes=nbytes, traffic_floor_ms=floor_ms, agreement_with_torch=agree,
                   speedup_over_torch=row["torch_conv2d"]["median_ms"] / row["image_metrics"]["median_ms"],
                   times_the_floor=row["image_metrics"]["median_ms"] / floor_ms)
        result["kernels"]["x".join(map(str, shape))] = row
        print(json.dumps({"shape": shape, **{k: row[k]["median_ms"] for k in t}, "floor_ms": floor_ms}), flush=True)
        del pred, target
        torch.cuda.empty_cache()

    # evaluate_views per view against render_image alone
    from nerf_amd import synthetic_weights as SW
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.utils import fov2Focal, pose_spherical
    nerf_amd.set_precision("bf16")
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(SW.proposal_state("small"))
    mip.load_state_dict(SW.mip_state("small"))
    prop, mip = prop.cuda().eval(), mip.cuda().eval()
    Vr, S = a.render_views, a.size
    focal = fov2Focal(0.6911112070083618, (S, S))
    poses = torch.stack([pose_spherical(360.0 * k / Vr, -30.0, 4.0)[:3] for k in range(Vr)]).cuda()
    images = torch.rand((Vr, 3, S, S), device="cuda", generator=gen)

    def renders():
        for v in range(Vr):
            procedures.render_image(mip, prop, poses[v], (S, S), focal, 2.0, 6.0, 128, white_bkg=True, seed=5 + v)

    def evaluated():
        metrics.evaluate_views(mip, prop, images, poses, focal, 2.0, 6.0, sample_num=128, white_bkg=True, seed=5)

    with torch.no_grad():
        renders()
        evaluated()
        torch.cuda.synchronize()
        t = alternate({"render_image": renders, "evaluate_views": evaluated}, 2, a.blocks)
    result["views"] = {k: {kk: (vv / Vr if kk.endswith("_ms") else vv) for kk, vv in summary(v).items()} for k, v in t.items()}
    result["views"].update(per="view", views=Vr, size=S, precision="bf16", sample_num=128)
    print(json.dumps(result["views"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
