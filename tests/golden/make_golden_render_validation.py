#!/usr/bin/env python3
"""Golden render_validation.json: what the four whole-ray render entry points and their four workspace queries ANSWER TO A CALL THAT FAILS A
CHECK -- (return code, message) -- as the commit before the entry points were folded into one pipeline answered it.  No GPU: every call is
made on host memory and is refused before any HIP call (or has N == 0 and returns before any launch), as in
tests/test_two_round_render_host.py.

    python tests/golden/make_golden_render_validation.py [OUTPUT.json]

Rows per entry point: every single fault of FAULTS that applies to it, the same fault in a call with N == 0, and pairs of faults.  A pair
records the two single rows it is made of: the test asks a pair for the same return code and the message of ONE of its two singles, so
that checks may be shared between the entry points without new messages.  tests/test_render_validation_host.py replays the rows."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LINEAR, DISPARITY = 0, 1
F32, BF16, BF16_F8, PROP_W128, FINE_W128 = 0, 1, 2, 0x100, 0x200

# argument names of the four entry points, in the order of include/nerf_amd.h
ARGS = {
    "nerf_amd_render_rays": ("packed_prop", "packed_fine", "precision", "rays", "camera", "ray_offset", "z_base", "u_strat", "u_inv", "N", "n_fine", "near", "far",
                             "white_bkg", "rgb", "depth", "weights", "workspace", "stream"),
    "nerf_amd_render_rays_warped": ("packed_prop", "packed_fine", "precision", "rays", "camera", "ray_offset", "u_strat", "u_inv", "N", "n_fine", "spacing", "near",
                                    "far", "white_bkg", "rgb", "depth", "weights", "workspace", "stream"),
    "nerf_amd_render_rays_rounds": ("packed_prop", "packed_fine", "precision", "rays", "camera", "ray_offset", "z_base", "N", "n_fine", "prop_pnum", "spacing", "near",
                                    "far", "white_bkg", "rgb", "depth", "weights", "workspace", "stream"),
    "nerf_amd_render_rays_ref": ("packed_prop", "packed_fine", "precision", "ref_flags", "rays", "camera", "ray_offset", "z_base", "u_strat", "u_inv", "N", "n_fine",
                                 "near", "far", "white_bkg", "cam_dir", "rgb", "depth", "normal_img", "workspace", "stream"),
}
POINTERS = ("packed_prop", "packed_fine", "rays", "z_base", "u_strat", "u_inv", "rgb", "depth", "weights", "workspace", "cam_dir", "normal_img")
# a call that passes every check of its entry point (variants: the rounds entry under either spacing)
BASE = dict(precision=F32, ref_flags=0, ray_offset=0, N=4, n_fine=64, prop_pnum=48, near=2.0, far=6.0, white_bkg=1, stream=None, weights=None)
VARIANTS = {
    "nerf_amd_render_rays": {"": {}},
    "nerf_amd_render_rays_warped": {"": dict(spacing=DISPARITY, near=0.2, far=1000.0)},
    "nerf_amd_render_rays_rounds": {"linear": dict(spacing=LINEAR), "disparity": dict(spacing=DISPARITY, near=0.2, far=1000.0)},
    "nerf_amd_render_rays_ref": {"": {}},
}


def _colliding_near_far():
    """near < far in fp32 whose reciprocals round to the same fp32"""
    for near in np.arange(1.25, 64.0, 0.25, dtype=np.float32):
        far = np.nextafter(near, np.float32(np.inf))
        if np.float32(1.0 / float(near)) == np.float32(1.0 / float(far)):
            return float(near), float(far)
    raise AssertionError("no colliding pair")


NEAR_C, FAR_C = _colliding_near_far()
IPE = {"cam.ipe": 1, "cam.ipe_radius": 0.01}
DISP = dict(spacing=DISPARITY, near=0.2, far=1000.0)
# name -> (changes, the (entry point, variant) pairs it applies to: a predicate on (entry, variant, argument names))
_all = lambda e, v, a: True                                                              # noqa: E731
_mip = lambda e, v, a: e != "nerf_amd_render_rays_ref"                                   # noqa: E731
_warped = lambda e, v, a: e == "nerf_amd_render_rays_warped" or v == "disparity"         # noqa: E731
_linear = lambda e, v, a: not _warped(e, v, a)                                           # noqa: E731
_has = lambda *names: (lambda e, v, a: all(n in a for n in names))                       # noqa: E731
_rounds = lambda e, v, a: e == "nerf_amd_render_rays_rounds"                             # noqa: E731
_both = lambda p, q: (lambda e, v, a: p(e, v, a) and q(e, v, a))                         # noqa: E731
FAULTS = {
    "packed_prop=NULL": (dict(packed_prop=None), _all),
    "packed_fine=NULL": (dict(packed_fine=None), _all),
    "z_base=NULL": (dict(z_base=None), _both(_has("z_base"), _linear)),
    "rgb=NULL": (dict(rgb=None), _all),
    "workspace=NULL": (dict(workspace=None), _all),
    "camera=NULL": (dict(camera=None), _rounds),
    "rays=NULL,camera=NULL": (dict(rays=None, camera=None), _has("u_strat")),
    "rays=NULL,no image": (dict(rays=None), _all),
    "N=-1": (dict(N=-1), _all),
    "n_fine=0": (dict(n_fine=0), _all),
    "n_fine=-1": (dict(n_fine=-1), _all),
    "n_fine=1024": (dict(n_fine=1024), _all),
    "prop_pnum=2": (dict(prop_pnum=2), _rounds),
    "prop_pnum=0": (dict(prop_pnum=0), _rounds),
    "prop_pnum=257": (dict(prop_pnum=257), _rounds),
    "spacing=2": (dict(spacing=2), _has("spacing")),
    "spacing=-1": (dict(spacing=-1), _has("spacing")),
    "spacing=linear": (dict(spacing=LINEAR), lambda e, v, a: e == "nerf_amd_render_rays_warped"),
    "near=0": (dict(near=0.0), _warped),
    "near=-1": (dict(near=-1.0), _warped),
    "far=near": (dict(near=2.0, far=2.0), _warped),
    "far=inf": (dict(far=float("inf")), _warped),
    "far=nan": (dict(far=float("nan")), _warped),
    "1/near=1/far": (dict(near=NEAR_C, far=FAR_C), _warped),
    "precision=7": (dict(precision=7), _all),
    "precision=-1": (dict(precision=-1), _all),
    "precision=F32|0x400": (dict(precision=F32 | 0x400), _all),
    "precision=BF16_F8": (dict(precision=BF16_F8), _all),
    "precision=BF16|FINE_W128 (ref)": (dict(precision=BF16 | FINE_W128), lambda e, v, a: e == "nerf_amd_render_rays_ref"),
    "ref_flags=2": (dict(ref_flags=2), _has("ref_flags")),
    "FINE_W128+ipe": (dict(precision=BF16 | FINE_W128, **IPE), _mip),
    "ipe,rays=NULL": (dict(rays=None, **{"cam.H": 4, "cam.W": 4}, **IPE), _both(_mip, _warped)),
    "ipe_radius=0": ({"cam.ipe": 1, "cam.ipe_radius": 0.0}, _mip),
    "ipe_radius=-1": ({"cam.ipe": 1, "cam.ipe_radius": -1.0}, _mip),
    "u_inv=NULL": (dict(u_inv=None), _has("u_strat")),
    "u_strat=NULL": (dict(u_strat=None), _has("u_strat")),
    "philox,camera=NULL": (dict(u_strat=None, u_inv=None, camera=None), _has("u_strat")),
    "normal_img without cam_dir": (dict(cam_dir=None), _has("cam_dir")),
    "cam_dir without normal_img": (dict(normal_img=None), _has("cam_dir")),
    "ray range past the image": (dict(rays=None, ray_offset=10, N=8, **{"cam.H": 4, "cam.W": 4}), _all),
    "ray_offset=-1": (dict(rays=None, ray_offset=-1, **{"cam.H": 4, "cam.W": 4}), _all),
    "lds: prop_pnum=256,n_fine=1023": (dict(prop_pnum=256, n_fine=1023), _rounds),
    "lds: prop_pnum=64,n_fine=800": (dict(prop_pnum=64, n_fine=800), _both(_rounds, _warped)),
    "lds: n_fine=800": (dict(n_fine=800), lambda e, v, a: e == "nerf_amd_render_rays_warped"),
    "lds: n_fine=1023": (dict(n_fine=1023), lambda e, v, a: e == "nerf_amd_render_rays_warped"),
}
# the faults that are paired with each other (every pair of them that applies to an entry point and touches different arguments)
PAIRED = ("packed_prop=NULL", "rgb=NULL", "workspace=NULL", "z_base=NULL", "camera=NULL", "rays=NULL,no image", "N=-1", "n_fine=0", "n_fine=1024", "prop_pnum=2",
          "prop_pnum=257", "spacing=2", "near=0", "far=near", "precision=7", "ref_flags=2", "FINE_W128+ipe", "ipe_radius=0", "u_inv=NULL", "philox,camera=NULL",
          "normal_img without cam_dir", "ray range past the image", "lds: prop_pnum=256,n_fine=1023", "lds: n_fine=800")
QUERIES = ("nerf_amd_render_workspace_bytes", "nerf_amd_render_warped_workspace_bytes", "nerf_amd_render_ref_workspace_bytes",
           "nerf_amd_render_rounds_workspace_bytes")
ROUNDS_GRID = [(N, F, P, sp) for N in (-1, 0, 1, 7, 1000, 640000) for F in (0, 1, 128, 1023) for P in (3, 64, 256) for sp in (LINEAR, DISPARITY)]


def rows():
    """-> [(key, entry point, variant, changes, singles)]: singles = the keys of the two single-fault rows a pair is made of, else None"""
    out = []
    for entry, names in ARGS.items():
        for variant in VARIANTS[entry]:
            applies = [f for f, (_, pred) in FAULTS.items() if pred(entry, variant, names)]
            head = "%s[%s] " % (entry, variant)
            for f in applies:
                out.append((head + f, entry, variant, FAULTS[f][0], None))
            for f in applies:
                if "N" not in FAULTS[f][0]:
                    out.append((head + f + " & N=0", entry, variant, dict(FAULTS[f][0], N=0), None))
            for f, g in itertools.combinations([f for f in PAIRED if f in applies], 2):
                a, b = FAULTS[f][0], FAULTS[g][0]
                if not set(a) & set(b):
                    out.append((head + f + " & " + g, entry, variant, dict(a, **b), (head + f, head + g)))
    return out


def call(_lib, entry, variant, changes):
    """-> (return code, message: "" for a call that returned 0) of the base call of (entry, variant) with `changes` applied"""
    bufs = {n: (C.c_float * 64)() for n in POINTERS}          # host memory: a call that got past the checks would fail in HIP
    cam = _lib.Samples()
    v = dict(BASE, camera=C.byref(cam), **{n: C.cast(b, C.c_void_p) for n, b in bufs.items() if n != "weights"})
    v.update(VARIANTS[entry][variant])
    for k, x in changes.items():
        if k.startswith("cam."):
            setattr(cam, k[4:], x)
        else:
            v[k] = x
    rc = getattr(_lib.lib, entry)(*[v[n] for n in ARGS[entry]])
    msg = _lib.lib.nerf_amd_last_error() if rc else b""
    return int(rc), (msg or b"").decode()


def queries(_lib):
    out = {}
    for name in QUERIES[:3]:
        out[name] = {"%d,%d" % (N, F): int(getattr(_lib.lib, name)(N, F)) for N in (-1, 0, 1, 7, 1000) for F in (-1, 0, 1, 128, 1023, 1024)}
    out[QUERIES[3]] = {"%d,%d,%d,%d" % a: int(_lib.lib.nerf_amd_render_rounds_workspace_bytes(*a))
                       for a in itertools.product((-1, 0, 1, 7, 1000), (0, 1, 128, 1023, 1024), (2, 3, 64, 256, 257), (-1, LINEAR, DISPARITY, 2))}
    return out


def rounds_workspace_table(_lib):
    return {"%d,%d,%d,%d" % a: int(_lib.lib.nerf_amd_render_rounds_workspace_bytes(*a)) for a in ROUNDS_GRID}


def main():
    sys.path.insert(0, ROOT)
    from nerf_amd import _lib
    table, dropped = {}, []
    for key, entry, variant, changes, singles in rows():
        rc, msg = call(_lib, entry, variant, changes)
        assert rc in (0, -1, -2) and (rc != 0 or changes.get("N") == 0), (key, rc, msg)      # refused by a check, never by HIP
        if singles and not (rc == table[singles[0]][0] == table[singles[1]][0] and msg in (table[singles[0]][1], table[singles[1]][1])):
            dropped.append((key, rc, msg))                                                   # the pair means something of its own: not a row
            continue
        table[key] = [rc, msg] + ([list(singles)] if singles else [])
    for d in dropped:
        print("not a row:", d)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "render_validation.json")
    json.dump({"calls": table, "queries": queries(_lib)}, open(path, "w"), indent=0, sort_keys=True)
    print("wrote %s: %d rows (%d pairs), %d bytes" % (path, len(table), sum(len(r) == 3 for r in table.values()), os.path.getsize(path)))
    ws = os.path.join(HERE, "render_workspace_bytes.json")
    sizes = json.load(open(ws))
    sizes["nerf_amd_render_rounds_workspace_bytes"] = rounds_workspace_table(_lib)
    json.dump(sizes, open(ws, "w"), indent=1, sort_keys=True)
    print("extended %s" % ws)


if __name__ == "__main__":
    main()
