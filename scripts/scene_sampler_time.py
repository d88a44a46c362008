#!/usr/bin/env python3
"""What scene mode costs or saves per training iteration: the MipNeRF TrainStep at 1 024 and 2^14 rays (64 + 128 samples, bf16), eager and
replayed from a hipGraph, in

  image mode   the reference's regime: a NEW 800 x 800 image and pose copied into the step every iteration (`step(img, pose)`), the
               captured step transposing it into a pixel table before it gathers the batch;
  scene mode   `TrainStep(scene=(images, poses))` over a synthetic stack of `--views` random 800 x 800 views, `step()` with no input.

Both steps start from the same parameters (tests/weights.py "small") with learning rate 0 (the Adam launch runs, the networks stay put, so
both modes time the same state), and are ALTERNATED in one process: `--repeats` rounds, each timing a window of `--iters` iterations per
mode between HIP events recorded at the iteration boundaries of a free-running loop (bench.py's timed_steps), after `--warmup` untimed
iterations.  A figure is the median over the rounds of the window medians; its spread is the range of the window medians.
The sampler alone: the scene launch against the image-mode pair (pixel-table transpose + sampler launch), each captured 50 times into one
hipGraph so that the figure is device time, not launch overhead.

    python scripts/scene_sampler_time.py --out profiles/scene_sampler_time.json --md profiles/scene_sampler_summary.md
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
H = W = 800
NEAR, FAR = 2.0, 6.0


def make_step(n_rays, c_n, f_n, focal, scene=None):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    import weights                                             # tests/weights.py: the closed-form "small" parameter sets of the tests
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.cuda().train(), mip.cuda().train()
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=0.0, lr_on_device=True)
    kw = {} if scene is None else {"scene": scene}
    return TrainStep(prop, mip, opt, (H, W), focal, NEAR, FAR, ray_num=n_rays, coarse_pnum=c_n, fine_pnum=f_n, seed=11, **kw)


def window(call, iters):
    """-> (per-iteration HIP-event times in ms, host wall ms per iteration) of `iters` calls without a synchronisation in between"""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(iters):
        call(i)
        evs[i + 1].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters * 1e3
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(iters)], wall


def figure(medians):
    return {"ms": statistics.median(medians), "min": min(medians), "max": max(medians), "windows": len(medians)}


def time_steps(n_rays, graph, images, poses, focal, a):
    st_img = make_step(n_rays, a.coarse, a.fine, focal)
    st_scn = make_step(n_rays, a.coarse, a.fine, focal, scene=(images, poses))
    V = images.shape[0]
    st_img.set_image(images[0], poses[0])
    if graph:
        st_img.capture(warmup=3)
        st_scn.capture(warmup=3)
    calls = {"image": lambda i: st_img(images[i % V], poses[i % V]),          # a new image every iteration, as train.py:153-157 has it
             "scene": lambda i: st_scn()}
    for c in calls.values():
        for i in range(a.warmup):
            c(i)
    gpu, wall = {"image": [], "scene": []}, {"image": [], "scene": []}
    for _ in range(a.repeats):
        for name, c in calls.items():
            g, w = window(c, a.iters)
            gpu[name].append(statistics.median(g))
            wall[name].append(w)
    out = {"image_ms": figure(gpu["image"]), "scene_ms": figure(gpu["scene"]), "image_wall_ms": figure(wall["image"]),
           "scene_wall_ms": figure(wall["scene"]), "loss_finite": bool(torch.isfinite(st_scn.loss).item() and torch.isfinite(st_img.loss).item())}
    spread = out["image_ms"]["max"] - out["image_ms"]["min"]
    out["image_spread_ms"] = spread
    out["scene_minus_image_ms"] = out["scene_ms"]["ms"] - out["image_ms"]["ms"]
    out["scene_not_slower_beyond_spread"] = bool(out["scene_minus_image_ms"] <= spread)
    return out


def time_sampler(n_rays, images, poses, focal, a, reps=50, replays=20):
    """device time of the batch draw alone, us per draw: `reps` draws captured into one hipGraph, `replays` timed replays"""
    from nerf_amd import ops
    from nerf_amd.utils import _focal_xy, randomFromOneImage
    fx, fy = _focal_xy(focal)
    seed = torch.full((1,), 11, dtype=torch.int64, device="cuda")
    img, pose = images[0], poses[0]

    def image_pair():
        pixels, coords = randomFromOneImage(img, (1.0, 1.0))
        return ops.sample_training_rays_dev(pixels, coords, pose, fx, fy, NEAR, FAR, n_rays, a.coarse, seed)

    def image_kernel_only(table=randomFromOneImage(img, (1.0, 1.0))):
        return ops.sample_training_rays_dev(table[0], table[1], pose, fx, fy, NEAR, FAR, n_rays, a.coarse, seed)

    def scene():
        return ops.sample_scene_rays(images, poses, fx, fy, NEAR, FAR, n_rays, a.coarse, seed_dev=seed)

    out = {}
    for name, fn in (("image_transpose_plus_sampler", image_pair), ("image_sampler_kernel_alone", image_kernel_only), ("scene_sampler", scene)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        ts, _ = window(lambda i: g.replay(), replays)
        out[name + "_us"] = {"us": statistics.median(ts) / reps * 1e3, "min": min(ts) / reps * 1e3, "max": max(ts) / reps * 1e3}
        del g
    return out


def markdown(res):
    L = ["# Scene-mode training step: measured", "",
         "`scripts/scene_sampler_time.py` on one MI355X: MipNeRF `TrainStep`, %d + %d samples, bf16, learning rate 0, image mode (a new 800 x 800 image"
         " copied in every iteration) and scene mode (%d views of 800 x 800, %.0f MB, no per-iteration input) alternated in one process; %d windows of %d"
         " iterations per mode; a figure is the median of the window medians of the per-iteration HIP-event times, [min, max] their range."
         % (res["coarse"], res["fine"], res["views"], res["views"] * 3 * H * W * 4 / 1e6, res["repeats"], res["iters"]), "",
         "| rays | replay | image mode ms [min, max] | scene mode ms [min, max] | scene - image ms | image-mode spread ms | not slower beyond the spread | host wall ms image / scene |",
         "|---|---|---|---|---|---|---|---|"]
    for key, e in res["steps"].items():
        n, mode = key.split("_")
        L.append("| %s | %s | %.4f [%.4f, %.4f] | %.4f [%.4f, %.4f] | %+.4f | %.4f | %s | %.4f / %.4f |"
                 % (n, mode, e["image_ms"]["ms"], e["image_ms"]["min"], e["image_ms"]["max"], e["scene_ms"]["ms"], e["scene_ms"]["min"], e["scene_ms"]["max"],
                    e["scene_minus_image_ms"], e["image_spread_ms"], "yes" if e["scene_not_slower_beyond_spread"] else "NO", e["image_wall_ms"]["ms"],
                    e["scene_wall_ms"]["ms"]))
    L += ["", "The batch draw alone (device time per draw, 50 draws captured in one hipGraph, median of 20 replays [min, max]):", "",
          "| rays | transpose + `train_sampler_kernel` us | `train_sampler_kernel` on a ready table us | `scene_sampler_kernel` us |", "|---|---|---|---|"]
    for n, e in res["sampler"].items():
        f = lambda x: "%.2f [%.2f, %.2f]" % (x["us"], x["min"], x["max"])
        L.append("| %s | %s | %s | %s |" % (n, f(e["image_transpose_plus_sampler_us"]), f(e["image_sampler_kernel_alone_us"]), f(e["scene_sampler_us"])))
    L += ["", "Image mode is the parent commit's code path (`randomFromOneImage` + `nerf_amd_sample_training_rays_dev`, results bit-identical).", ""]
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 1 << 14])
    ap.add_argument("--coarse", type=int, default=64)
    ap.add_argument("--fine", type=int, default=128)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--iters", type=int, default=60, help="timed iterations per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5, help="windows per mode (>= 5: the spread of the image-mode figure is the yardstick)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_sampler_time.py: needs a GPU (a CPU run measures nothing)")
    import nerf_amd
    from oracle import nerf_oracle as O                        # (pose / focal helpers only; nothing timed)
    nerf_amd.set_precision("bf16")
    gen = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand(a.views, 3, H, W, device="cuda", generator=gen)
    poses = torch.stack([O.pose_spherical(360.0 * v / a.views, -30.0, 4.0)[:3] for v in range(a.views)]).contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, W))
    res = {"coarse": a.coarse, "fine": a.fine, "views": a.views, "iters": a.iters, "repeats": a.repeats, "warmup": a.warmup, "steps": {}, "sampler": {}}
    for n in a.rays:
        for graph in (False, True):
            key = "%d_%s" % (n, "hipgraph" if graph else "eager")
            res["steps"][key] = time_steps(n, graph, images, poses, focal, a)
            print(key, json.dumps(res["steps"][key]), flush=True)
            torch.cuda.empty_cache()
        res["sampler"][str(n)] = time_sampler(n, images, poses, focal, a)
        print("sampler", n, json.dumps(res["sampler"][str(n)]), flush=True)
    line = json.dumps(res)
    print(line)
    for path, text in ((a.out, line + "\n"), (a.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
