#!/usr/bin/env python3
"""Do the persistent workgroups of the two render MLP kernels finish together?  (profiles/elastic_tiles_probe.md)

Needs the diagnostic libraries of `-DMLP_TILEPROBE` (mlp_kernels.hip), one per kernel family:

    make -C nerf_amd/csrc variant_tu NAME=TILEPROBE_PROP TU=1 FLAGS=-DMLP_TILEPROBE
    make -C nerf_amd/csrc variant_tu NAME=TILEPROBE_MIP  TU=2 FLAGS=-DMLP_TILEPROBE
    python scripts/gpu_tile_probe.py [--lib-suffix _ELASTIC] [--base-lib PATH] [--append]

For each of the two it runs the bench command in a process of its own with the library named through NERF_AMD_LIB -- bench.py itself, in
that process, so that the probe's buffer can be read once the run has ended -- long enough for the last launches to come after more than
2 s of back-to-back steps, and takes the last three full-size launches out of the buffer: per workgroup the 100 MHz real-time stamps and
shader-clock stamps at kernel entry and after the weight stream's drain, its XCD and its tile count.  It also runs the plain bench
command three times on the shipped library (or --base-lib) for the run-to-run spread of roofline.ms_per_launch, and writes

    potential = (last finish - mean finish) / kernel duration        (what a perfect hand-out of the tiles could take off a launch)

next to twice that spread into profiles/elastic_tiles_probe.md (--append: a further box or library under the text that is there).
Every run has a time limit of its own and the script stops at the first one that fails."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES, WGS = 8, 1024                      # TILEPROBE_LAUNCHES, TILEPROBE_WGS of mlp_kernels.hip
QUIET = ["--no-cpu-baseline", "--no-train-rate", "--no-gemm-ref"]       # (skip measurements outside the timed region only)
KERNELS = {"mip": ("TILEPROBE_MIP", "mip_kernel<PBF16WR,false> (fine)", "roofline"),
           "prop": ("TILEPROBE_PROP", "proposal_kernel<PBF16WR,false>", "roofline_proposal")}


class Rec(ctypes.Structure):
    """struct TileProbeRec"""
    _fields_ = [("real0", ctypes.c_uint64), ("real1", ctypes.c_uint64), ("clk0", ctypes.c_uint64), ("clk1", ctypes.c_uint64),
                ("xcc", ctypes.c_uint32), ("tiles", ctypes.c_uint32), ("grid", ctypes.c_uint32), ("seq", ctypes.c_uint32)]


def child(kernel, steps, warmup, raw_path):
    """bench.py in THIS process (NERF_AMD_LIB is set by the parent), then the probe's buffer"""
    import contextlib
    import io
    import runpy
    sys.path.insert(0, ROOT)
    sys.argv = ["bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)] + QUIET
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        except SystemExit as e:
            if e.code not in (None, 0):
                raise
    line = [ln for ln in out.getvalue().splitlines() if ln.startswith("{")][-1]
    from nerf_amd import _lib
    buf = (Rec * (LAUNCHES * WGS))()
    rc = getattr(_lib.lib, "nerf_amd_tileprobe_read_" + kernel)(ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_size_t(ctypes.sizeof(buf)))
    if rc != 0:
        sys.exit("nerf_amd_tileprobe_read_%s failed (%d)" % (kernel, rc))
    launches = []
    for slot in range(LAUNCHES):
        grid, seq = buf[slot * WGS].grid, buf[slot * WGS].seq
        if grid == 0 or grid > WGS:
            continue
        recs = [buf[slot * WGS + i] for i in range(grid)]
        if any(r.seq != seq or r.grid != grid for r in recs):
            continue                                            # (a slot that a smaller launch has partly overwritten)
        launches.append({"seq": seq, "grid": grid, "wg": [[r.real0, r.real1, r.clk0, r.clk1, r.xcc, r.tiles] for r in recs]})
    with open(raw_path, "w") as f:
        json.dump({"bench": json.loads(line), "launches": sorted(launches, key=lambda l: l["seq"])}, f)


def run(cmd, env, limit):
    print("+ " + " ".join(cmd), flush=True)
    p = subprocess.run(cmd, env=env, cwd=ROOT, timeout=limit, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit("gpu_tile_probe: `%s` ended with status %d -- stopping" % (" ".join(cmd), p.returncode))
    return p.stdout


def analyse(launch):
    wg = launch["wg"]
    start, end = min(w[0] for w in wg), max(w[1] for w in wg)
    first_end = min(w[1] for w in wg)
    dur = (end - start) / 100.0                                 # us (100 MHz ticks)
    mean_end = statistics.fmean(w[1] for w in wg)
    by_xcd = {}
    for w in wg:
        by_xcd.setdefault(w[4], []).append(w)
    rows = []
    for x in sorted(by_xcd):
        ws = by_xcd[x]
        fin = [(w[1] - first_end) / 100.0 for w in ws]
        mhz = [(w[3] - w[2]) / max(w[1] - w[0], 1) * 100.0 for w in ws]
        rows.append({"xcd": x, "n": len(ws), "fin_min": min(fin), "fin_mean": statistics.fmean(fin), "fin_max": max(fin), "mhz": statistics.fmean(mhz),
                     "tiles_min": min(w[5] for w in ws), "tiles_max": max(w[5] for w in ws), "start_max": max((w[0] - start) / 100.0 for w in ws)})
    return {"seq": launch["seq"], "grid": launch["grid"], "tiles": sum(w[5] for w in wg), "duration_us": dur, "spread_us": (end - first_end) / 100.0,
            "potential": (end - mean_end) / 100.0 / dur, "xcd": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, choices=list(KERNELS))
    ap.add_argument("--raw", default=None)
    ap.add_argument("--raw-dir", default=None, help="keep the raw per-workgroup records (JSON, one file per kernel) here; default: a temporary directory")
    ap.add_argument("--steps", type=int, default=40, help="probe runs: 40 + 5 steps of ~67 ms put the last launches behind 2.8 s of steps")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lib-suffix", default="", help="probe libraries nerf_amd/ablate/libnerf_amd_TILEPROBE_{MIP,PROP}<suffix>.so")
    ap.add_argument("--base-lib", default=None, help="library of the three plain runs (default: the shipped one)")
    ap.add_argument("--label", default="", help="heading of this section")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_tiles_probe.md"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="time limit of each run, seconds")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup, a.raw)

    raw_dir = os.path.abspath(a.raw_dir) if a.raw_dir else tempfile.mkdtemp(prefix="tile_probe_")
    os.makedirs(raw_dir, exist_ok=True)
    env = dict(os.environ)
    env.pop("NERF_AMD_LIB", None)
    if a.base_lib:
        env["NERF_AMD_LIB"] = os.path.abspath(a.base_lib)
    plain = []
    for _ in range(3):                                          # the yardstick's own run-to-run spread, same session
        out = run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + QUIET, env, a.limit)
        plain.append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
    spread = {}
    for k, (_, _, key) in KERNELS.items():
        v = [r[key]["ms_per_launch"] for r in plain]
        spread[k] = {"runs": v, "frac": (max(v) - min(v)) / statistics.fmean(v)}

    res = {}
    for k, (name, _, _) in KERNELS.items():
        lib = os.path.join(ROOT, "nerf_amd", "ablate", "libnerf_amd_%s%s.so" % (name, a.lib_suffix))
        raw = os.path.join(raw_dir, "tile_probe_%s%s.json" % (k, a.lib_suffix))
        run([sys.executable, os.path.abspath(__file__), "--child", k, "--raw", raw, "--steps", str(a.steps), "--warmup", str(a.warmup)],
            dict(env, NERF_AMD_LIB=lib), a.limit)
        with open(raw) as f:
            d = json.load(f)
        full = max(sum(w[5] for w in l["wg"]) for l in d["launches"])
        launches = [analyse(l) for l in d["launches"] if sum(w[5] for w in l["wg"]) == full][-3:]       # the last three full-size launches
        res[k] = {"launches": launches, "bench_ms": d["bench"][KERNELS[k][2]]["ms_per_launch"]}

    try:
        import torch
        dev = torch.cuda.get_device_properties(0)
        box = "%s, %d CUs" % (dev.name, dev.multi_processor_count)
    except Exception:                                           # noqa: BLE001
        box = "unknown device"
    L = []
    if not (a.append and os.path.exists(a.out)):
        L += ["# Render MLP kernels: do the persistent workgroups finish together?", "",
              "Written by `scripts/gpu_tile_probe.py` (libraries built with `-DMLP_TILEPROBE`, `make variant_tu`).  Every workgroup of",
              "`proposal_kernel<PBF16WR,false>` and `mip_kernel<PBF16WR,false>` stamps the 100 MHz real-time counter and the shader clock counter",
              "at kernel entry and after the weight stream's drain; its XCD and tile count go with them into a buffer of the probe's own.",
              "Finish times are relative to the launch's first workgroup to finish; `potential = (last finish - mean finish) / kernel duration`",
              "is what a perfect hand-out of the tiles could take off a launch, to be set against twice the run-to-run spread (max - min over",
              "mean) of the bench's `ms_per_launch` over three plain runs of the same session.", ""]
    L += ["## %s" % (a.label or box), "", "Box: %s.  Probe runs: `bench.py --gpus 1 --steps %d --warmup %d`, the last three full-size launches." % (box, a.steps, a.warmup), ""]
    for k, (_, title, _) in KERNELS.items():
        sp = spread[k]
        pots = [l["potential"] for l in res[k]["launches"]]
        L += ["### %s" % title, "",
              "Plain runs, `ms_per_launch`: %s -> spread %.3f %%, twice that %.3f %%.  Probe run: %.3f ms per launch." %
              (" / ".join("%.3f" % v for v in sp["runs"]), 100 * sp["frac"], 200 * sp["frac"], res[k]["bench_ms"]),
              "`potential`: %s -> %s twice the spread in %d of %d launches." %
              (" / ".join("%.3f %%" % (100 * p) for p in pots), "above" if min(pots) > 2 * sp["frac"] else "not above",
               sum(p > 2 * sp["frac"] for p in pots), len(pots)), ""]
        for l in res[k]["launches"]:
            L += ["Launch %d: %d workgroups, %d tiles, %.1f us from first entry to last finish; first to last finish %.1f us; potential %.3f %%." %
                  (l["seq"], l["grid"], l["tiles"], l["duration_us"], l["spread_us"], 100 * l["potential"]), "",
                  "| XCD | workgroups | tiles per workgroup | latest entry, us | finish min / mean / max, us | in-kernel clock, MHz |", "|---|---|---|---|---|---|"]
            for x in l["xcd"]:
                L.append("| %d | %d | %s | %.1f | %.1f / %.1f / %.1f | %.0f |" % (
                    x["xcd"], x["n"], ("%d" % x["tiles_min"]) if x["tiles_min"] == x["tiles_max"] else "%d-%d" % (x["tiles_min"], x["tiles_max"]),
                    x["start_max"], x["fin_min"], x["fin_mean"], x["fin_max"], x["mhz"]))
            L.append("")
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))
    print(json.dumps({"spread": spread, "potential": {k: [l["potential"] for l in v["launches"]] for k, v in res.items()}}))


if __name__ == "__main__":
    main()
