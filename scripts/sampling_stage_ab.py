#!/usr/bin/env python3
"""Two builds of sample_kernels.hip against each other: every op whose kernel holds one of the shared per-ray stages (the resampling rows
and stages, the merge searches, the block sums, camera_ray, point_on_ray) on seeded inputs at the benchmark's shape -- 640 000 rays of an
800 x 800 camera, C = 64 coarse and K = 129 fine samples, in-kernel Philox uniforms -- with the SHA-256 of every output's bytes.

    python scripts/sampling_stage_ab.py --out new.json                                    # this tree's library
    NERF_AMD_LIB=/path/to/parent/libnerf_amd.so python scripts/sampling_stage_ab.py --out parent.json
    python scripts/sampling_stage_ab.py --compare parent.json new.json                    # every hash must be equal

(the ABI is unchanged, so this tree's package drives either library).  Kernel times: `--repeat R --no-hash` launches every op R times;
run that under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o kt -- python scripts/sampling_stage_ab.py ...`, one
process per run, the two libraries alternated, then

    python scripts/sampling_stage_ab.py --compare-stats parent_1/ parent_2/ ... : new_1/ new_2/ ...

prints, per touched kernel, the median and the spread (max - min) of the per-run mean durations and applies the rule: the new median may
exceed the parent's by no more than the parent's own spread."""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SIDE, C, K, P, NF = 800, 64, 129, 64, 128
NEAR, FAR = 2.0, 6.0
WNEAR, WFAR = 0.2, 1000.0
SEED = 20240607
TOUCHED = ("resample_kernel", "warped_resample_kernel", "resample_window_kernel<false>", "resample_window_kernel<true>", "inverse_sample_kernel",
           "max_blur_kernel", "merge_sorted_kernel", "merge_sorted_order_kernel", "raygen_kernel", "pixel_rays_kernel", "stratified_points_kernel",
           "warp_depths_kernel", "warped_stratified_kernel", "scene_sampler_kernel", "weighted_dot_loss_kernel", "weighted_dot_loss_final_kernel",
           "distortion_loss_kernel<0>", "distortion_loss_kernel<1>", "distortion_loss_final_kernel", "interlevel_loss_kernel",
           "interlevel_loss_final_kernel")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("sampling_stage_ab.py: needs a GPU")
    import nerf_amd
    import weights
    from nerf_amd import ops, utils
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from oracle import nerf_oracle as O                        # (pose / focal helpers only)
    nerf_amd.set_precision("bf16")
    dev = torch.device("cuda", 0)
    N = SIDE * SIDE
    hashes = {}

    def rec(name, fn, pick=None):
        """call the op a.repeat times; hash the tensors of its last result"""
        for _ in range(a.repeat):
            r = fn()
        r = pick(r) if pick else (r if isinstance(r, (tuple, list)) else (r,))
        torch.cuda.synchronize()
        if not a.no_hash:
            for i, t in enumerate(r):
                if isinstance(t, torch.Tensor):
                    hashes["%s.%d" % (name, i)] = sha(t)
        print(name, "done", flush=True)
        return r

    g = torch.Generator(device="cuda").manual_seed(SEED)
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().to(dev)
    fx, fy = utils._focal_xy(O.fov2focal(0.6911112070083618, (SIDE, SIDE)))
    rays, = rec("generate_rays", lambda: ops.generate_rays(pose, SIDE, SIDE, fx, fy, dev))
    coords = torch.stack((torch.randint(-SIDE // 2, SIDE // 2, (N,), device=dev, generator=g),
                          torch.randint(-SIDE // 2, SIDE // 2, (N,), device=dev, generator=g)), -1).contiguous()
    rec("pixel_rays", lambda: ops.pixel_rays(coords, pose, fx, fy))
    z_base = torch.linspace(NEAR, FAR, C, device=dev)
    jitter = (FAR - NEAR) / NF
    u_strat = ops.philox_stream((N, C), SEED, 0, strat=True, device=dev)
    u_inv = ops.philox_stream((N, K), SEED, 0, device=dev)
    density = torch.randn(N, C, device=dev, generator=g) * 2.0
    z_c, _ = rec("stratified_points", lambda: ops.stratified_points(rays, z_base, u_strat, jitter))
    s_c, _, _ = rec("warped_stratified", lambda: ops.warped_stratified(rays, None, WNEAR, WFAR, n_points=C, seed=SEED))
    rec("warp_depths", lambda: ops.warp_depths(s_c, WNEAR, WFAR, rays))
    z_f, below, w_prop, _ = rec("resample", lambda: ops.resample(density, None, z_base, None, jitter, rays, None, K, want_below=True, want_w=True, want_zc=True,
                                                                 seed=SEED))
    rec("warped_resample", lambda: ops.warped_resample(density, s_c, rays, None, WNEAR, WFAR, K=K, seed=SEED))
    w_raw = ops.sigma_to_weights(density, z_c, rays[:, 3:].contiguous())
    rec("max_blur", lambda: ops.max_blur(w_raw, 0.01))
    rec("inverse_sample", lambda: ops.inverse_sample(w_prop, z_c, u_inv, sort=True))
    rec("sample_pdf", lambda: ops.sample_pdf(z_c, w_prop[:, :-1].contiguous(), u_inv))
    rec("merge_depths", lambda: ops.merge_depths(z_f, z_c))
    rec("merge_depths_order", lambda: ops.merge_depths_order(z_f, z_c, below))
    images = torch.rand(4, 3, 96, 128, device=dev, generator=g)
    poses = torch.stack([O.pose_spherical(90.0 * v, -30.0, 4.0)[:3] for v in range(4)]).contiguous().to(dev)
    rec("sample_scene_rays", lambda: ops.sample_scene_rays(images, poses, fx, fy, NEAR, FAR, N, C, seed=SEED))
    # the three losses, forward: fine weights over the fine depths, the proposal histogram over the coarse depths
    w_fine = ops.sigma_to_weights(torch.randn(N, K, device=dev, generator=g) * 2.0, z_f, rays[:, 3:].contiguous())
    nrm = torch.nn.functional.normalize(torch.randn(N * C, 3, device=dev, generator=g), dim=-1)
    nrm2 = torch.nn.functional.normalize(torch.randn(N * C, 3, device=dev, generator=g), dim=-1)
    for mode in (0, 1):
        rec("weighted_dot_loss.%d" % mode, lambda: ops.weighted_dot_loss(w_raw.reshape(-1), nrm, nrm2, mode, 1.0 / (N * C)))
    rec("distortion_loss.0", lambda: ops.distortion_loss(w_fine, z_f, 0, 1.0))
    rec("distortion_loss.1", lambda: ops.distortion_loss(w_fine[:, :-1].contiguous(), z_f, 1, 1.0))
    rec("interlevel_loss", lambda: ops.interlevel_loss(w_fine[:, :-1].contiguous(), z_f, w_prop, z_c, 1.0, want_bounds=True))
    # the window kernels: round two of the two-round render, both spacings
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(weights.proposal_state("small"))
    mip.load_state_dict(weights.mip_state("small"))
    prop, mip = prop.to(dev).eval(), mip.to(dev).eval()
    pk_p, pk_m = prop.packed(ops.BF16), mip.packed(ops.BF16)
    for spacing, near, far, contract in (("linear", NEAR, FAR, False), ("disparity", WNEAR, WFAR, True)):
        zb = torch.linspace(near, far, 64, device=dev)
        with torch.no_grad():
            rec("render_rays_rounds.%s" % spacing,
                lambda: ops.render_rays_rounds(pk_p, pk_m, ops.BF16, rays, zb, NF, near, far, True, prop_pnum=P, seed=SEED, spacing=spacing, contract=contract,
                                               want_fine_depths=True),
                pick=lambda r: (r[0], r[1], r[4]["fine_depths"]))
    res = {"library": os.environ.get("NERF_AMD_LIB") or "in-tree", "rays": N, "C": C, "K": K, "repeat": a.repeat, "sha256": hashes}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "sha256"}), "%d outputs hashed" % len(hashes))


def compare(pa, pb):
    a, b = (json.load(open(p))["sha256"] for p in (pa, pb))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in sorted(a):
        print("%-34s %s  %s" % (k, a[k][:16], "equal" if k not in bad else "DIFFERENT (%s)" % str(b.get(k))[:16]))
    print("%d outputs, %d different" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad or not a else 0


def kernel_means(d):
    """{short kernel name: mean duration in us} of the one *_kernel_stats.csv under directory d"""
    path, = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    out = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"\(anonymous namespace\)::", "", r["Name"])
        name = re.sub(r"\(.*$", "", re.sub(r"^void ", "", name))
        out[name] = float(r["AverageNs"]) / 1e3
    return out


def compare_stats(parent_dirs, new_dirs):
    par, new = [kernel_means(d) for d in parent_dirs], [kernel_means(d) for d in new_dirs]
    print("| kernel | parent median us | parent max - min us | new median us | new max - min us | new - parent us | within the parent's spread |")
    print("|---|---|---|---|---|---|---|")
    worst = 0
    for k in TOUCHED:
        p, n = [m[k] for m in par if k in m], [m[k] for m in new if k in m]
        if not p or not n:
            print("| `%s` | not launched | | | | | |" % k)
            continue
        pm, nm, ps = statistics.median(p), statistics.median(n), max(p) - min(p)
        ok = nm - pm <= ps
        worst |= 0 if ok else 1
        print("| `%s` | %.2f | %.2f | %.2f | %.2f | %+.2f | %s |" % (k, pm, ps, nm, max(n) - min(n), nm - pm, "yes" if ok else "NO"))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file for the hashes")
    ap.add_argument("--repeat", type=int, default=1, help="launches per op (kernel timing under rocprofv3)")
    ap.add_argument("--no-hash", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_JSON", "NEW_JSON"))
    ap.add_argument("--compare-stats", nargs="+", metavar="DIR", help="rocprofv3 output directories: PARENT... : NEW... (a lone ':' separates)")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.compare_stats:
        i = a.compare_stats.index(":")
        sys.exit(compare_stats(a.compare_stats[:i], a.compare_stats[i + 1:]))
    run(a)


if __name__ == "__main__":
    main()
