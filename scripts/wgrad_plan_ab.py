#!/usr/bin/env python3
"""Two builds of the training backward's host side (nerf_amd/csrc/bwd_kernels.hip) against each other: nerf_amd_proposal_weight_grads,
nerf_amd_mip_weight_grads and nerf_amd_ref_backward on the cases of tests/test_gpu_wgrad_plan.py plus one per network at the
benchmark's 16 384 rays per step (bf16: 64 coarse samples per ray for the proposal network, 128 fine ones for MipNeRF, 192 merged ones
for Ref-NeRF), each on a zero-filled workspace of exactly the queried size.  Per case: the SHA-256 of every gradient tensor (the
arithmetic) and a position-weighted 64-bit checksum of the whole workspace after the call (the layout of the parts and the workgroup
count of every batch: a partial that moved, or one workgroup more or less, changes it).

    python scripts/wgrad_plan_ab.py --out new.json                                     # this tree's library
    NERF_AMD_LIB=/path/to/parent/libnerf_amd.so python scripts/wgrad_plan_ab.py --out parent.json
    python scripts/wgrad_plan_ab.py --compare parent.json new.json                     # every line must be equal

(the ABI is unchanged, so this tree's package drives either library)."""
import argparse
import gc
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BENCH_RAYS = 16384
BENCH_SAMPLES = {"prop": 64, "mip": 128, "ref": 192}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def checksum(ws):
    """(sum of the 64-bit words, sum of word x (2 index + 1)) mod 2^64, on the device, a GiB at a time"""
    import torch
    words = ws[: ws.numel() // 8 * 8].view(torch.int64)
    s0 = s1 = 0
    step = 1 << 27
    for lo in range(0, words.numel(), step):
        w = words[lo: lo + step]
        s0 += int(w.sum())
        s1 += int((w * (2 * torch.arange(lo, lo + w.numel(), device=w.device) + 1)).sum())
    tail = ws[ws.numel() // 8 * 8:]
    return "%016x%016x+%s" % (s0 % (1 << 64), s1 % (1 << 64), tail.cpu().numpy().tobytes().hex())


def run(a):
    import torch
    if not torch.cuda.is_available():
        sys.exit("wgrad_plan_ab.py: needs a GPU")
    import test_gpu_wgrad_plan as T
    A = T.make_namespace()
    cases = [(n, p, f, M) for n in ("prop", "mip") for p, f in T.PM_MODES for M in T.SIZES]
    cases += [("ref", p, "bf16", M) for p in ("fp32", "bf16") for M in T.SIZES]
    cases += [(n, "bf16", "bf16", BENCH_RAYS * s) for n, s in BENCH_SAMPLES.items()]
    res = {}
    for name, prec, fmt, M in cases:
        need, call = T.prepare(A, name, prec, fmt, M)
        ws = T.RF._filled(need, 0x00)
        grads = call(ws, 0x00)
        torch.cuda.synchronize()
        key = "%s %s %s-dumps M=%d" % (name, prec, fmt, M)
        res[key] = {"workspace_bytes": int(need), "workspace": checksum(ws)}
        res[key].update({k: sha(g) for k, g in sorted(grads.items())})
        print(key, "done: %d bytes, %d tensors" % (need, len(grads)), flush=True)
        del ws, grads, call
        gc.collect()
        torch.cuda.empty_cache()
    out = {"library": os.environ.get("NERF_AMD_LIB") or "in-tree", "compute_units": A.n_cu, "cases": res}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"library": out["library"], "compute_units": A.n_cu, "cases": len(res), "hashes": sum(len(v) - 1 for v in res.values())}))


def compare(pa, pb):
    a, b = (json.load(open(p))["cases"] for p in (pa, pb))
    n = bad = 0
    for case in sorted(set(a) | set(b)):
        ca, cb = a.get(case, {}), b.get(case, {})
        diff = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
        n += len(set(ca) | set(cb))
        bad += len(diff)
        print("%-40s %3d entries  %s" % (case, len(ca), "equal" if not diff else "DIFFERENT: " + ", ".join(diff)))
    print("%d cases, %d entries, %d different" % (len(set(a) | set(b)), n, bad))
    return 1 if bad or not a else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="JSON file for the hashes")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_JSON", "NEW_JSON"))
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    run(a)


if __name__ == "__main__":
    main()
