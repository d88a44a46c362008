#!/usr/bin/env python3
"""Cost of the iso-surface extraction (nerf_amd_mesh_count / nerf_amd_mesh_emit) and of density_grid, on the GPU.

  default          HIP-event times of the two calls and of marching_tetrahedra as a whole (host read of the counts included) on a
                   sphere field and a white-noise field at 256^3 and 512^3, then density_grid (MipNeRF, bf16, the closed-form "small"
                   weights) at the same resolutions, and the lattice passes as a fraction of it.  Writes one JSON to --out.
                   White noise at 512^3 has more than 2^31 / 3 triangles: the emit is refused there by definition, the count pass is
                   timed, and a smooth noise (64^3 noise, trilinear x 8) stands in for the emit.
  --trace-run      a few calls per field and nothing else: run it under `rocprofv3 --kernel-trace --output-format csv -d DIR -o kt --`
  --summarize DIR  per-kernel medians of that trace, with the bytes each kernel must move: one read of the field, the byte / prefix /
                   tile traffic, the output.

    python scripts/gpu_mesh_rate.py --out profiles/mesh_extraction_rate.json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 5
KERNELS = ("mesh_classify_kernel", "mesh_scan_kernel", "mesh_vertex_kernel", "mesh_face_kernel")


def fields(torch, sizes):
    """(name, n, make): device fields (n, n, n), made on demand"""
    def sphere(n):
        ax = torch.arange(n, device="cuda", dtype=torch.float32) - 0.5 * (n - 1) + 0.1
        return ((0.33 * n) ** 2 - (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).contiguous()

    def noise(n):
        return torch.randn((n, n, n), device="cuda", generator=torch.Generator(device="cuda").manual_seed(n))

    def smooth(n):
        low = torch.randn((1, 1, n // 8, n // 8, n // 8), device="cuda", generator=torch.Generator(device="cuda").manual_seed(n + 1))
        return torch.nn.functional.interpolate(low, scale_factor=8, mode="trilinear", align_corners=False)[0, 0].contiguous()

    out = []
    for n in sizes:
        out += [("sphere", n, sphere), ("noise", n, noise)]
        if n >= 512:
            out.append(("smooth noise", n, smooth))
    return out


def time_ms(torch, fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def traffic(n, V, F, normals=True):
    """bytes each kernel must move at n points, V vertices, F faces"""
    tiles = (n + 255) // 256
    return {"mesh_classify_kernel": 4 * n + n + 8 * tiles, "mesh_scan_kernel": 16 * tiles,
            "mesh_vertex_kernel": n + 4 * n + 4 * tiles + (24 if normals else 12) * V, "mesh_face_kernel": n + 4 * tiles + 12 * F}


def emit_allowed(V, F):
    return V < 2 ** 31 and 3 * F < 2 ** 31


def run_fields(torch, ops, sizes, trace):
    rows = []
    for name, n, make in fields(torch, sizes):
        f = make(n)
        counts, ws = ops.mesh_count(f, 0.0)
        V, F = (int(c) for c in counts.tolist())
        ok = emit_allowed(V, F)
        row = {"field": name, "n": n, "points": n ** 3, "vertices": V, "faces": F, "emit": ok}
        if ok:
            out = ops.mesh_emit(f, 0.0, ws, V, F)                                  # warm; also holds the outputs' memory
        torch.cuda.synchronize()
        if trace:
            for _ in range(REPEATS):
                ops.mesh_count(f, 0.0)
                if ok:
                    ops.mesh_emit(f, 0.0, ws, V, F)
            torch.cuda.synchronize()
        else:
            from nerf_amd import mesh
            row["count_ms"] = [time_ms(torch, lambda: ops.mesh_count(f, 0.0), 3) for _ in range(REPEATS)]
            if ok:
                row["emit_ms"] = [time_ms(torch, lambda: ops.mesh_emit(f, 0.0, ws, V, F), 3) for _ in range(REPEATS)]
                del out
                row["marching_tetrahedra_ms"] = [time_ms(torch, lambda: mesh.marching_tetrahedra(f, 0.0), 1) for _ in range(REPEATS)]
            row["bytes"] = traffic(n ** 3, V, F)
        rows.append(row)
        print(json.dumps({k: (statistics.median(v) if isinstance(v, list) else v) for k, v in row.items() if k != "bytes"}), flush=True)
        out = None
        del f, ws
        torch.cuda.empty_cache()
    return rows


def summarize(trace_dir, sizes):
    """per (field, kernel): median [min, max] us of the REPEATS traced calls behind one warm call, and GB/s over the bytes of traffic()"""
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert path, "no *kernel_trace.csv under %s" % trace_dir
    calls = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(path[0])):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                calls[k].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    shapes = json.load(open(os.path.join(trace_dir, "fields.json")))
    out = []
    at = {k: 0 for k in KERNELS}
    for k in KERNELS:
        calls[k].sort()
    for row in shapes:
        per = {}
        for k in KERNELS:
            if not row["emit"] and k in ("mesh_vertex_kernel", "mesh_face_kernel"):
                continue
            us = [d for _, d in calls[k][at[k]:at[k] + REPEATS + 1]][1:]             # the first call of a field is its warm-up
            at[k] += REPEATS + 1
            nbytes = traffic(row["points"], row["vertices"], row["faces"])[k]
            per[k] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "bytes": nbytes, "gb_per_s": nbytes / (statistics.median(us) * 1e-6) / 1e9}
        out.append(dict(row, kernels=per))
    assert all(at[k] == len(calls[k]) for k in KERNELS), "the trace holds other calls than the ones of --trace-run"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--trace-run", default=None, metavar="DIR", help="run the traced calls only; fields.json goes to DIR")
    ap.add_argument("--summarize", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.summarize:
        result = summarize(a.summarize, a.sizes)
        print(json.dumps(result, indent=1))
        if a.out:
            json.dump(result, open(a.out, "w"), indent=1)
        return
    import torch
    assert torch.cuda.is_available(), "this script measures on the GPU; there is nothing to measure without one"
    import nerf_amd
    from nerf_amd import mesh, ops
    if a.trace_run:
        rows = run_fields(torch, ops, a.sizes, trace=True)
        os.makedirs(a.trace_run, exist_ok=True)
        json.dump(rows, open(os.path.join(a.trace_run, "fields.json"), "w"))
        return
    result = {"device": torch.cuda.get_device_name(0), "fields": run_fields(torch, ops, a.sizes, trace=False), "density_grid": []}
    from nerf_amd import synthetic_weights as SW
    from nerf_amd.mip_model import MipNeRF
    nerf_amd.set_precision("bf16")
    mip = MipNeRF(10, 4, 256)
    mip.load_state_dict(SW.mip_state("small"))
    mip = mip.cuda().eval()
    box = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    mesh.density_grid(mip, box, 64)                                              # warm: packs the weights
    for n in a.sizes:
        ms = [time_ms(torch, lambda: mesh.density_grid(mip, box, n), 1) for _ in range(3)]
        lattice = [statistics.median(r["count_ms"]) + statistics.median(r.get("emit_ms", [0.0])) for r in result["fields"] if r["n"] == n and r["emit"]]
        row = {"n": n, "points": n ** 3, "density_grid_ms": ms, "points_per_s": n ** 3 / (statistics.median(ms) * 1e-3),
               "lattice_passes_ms": lattice, "lattice_fraction_of_density_grid": [v / statistics.median(ms) for v in lattice]}
        result["density_grid"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(result, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
