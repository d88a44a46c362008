"""Depth quantiles and opacity without a GPU: the fp64 specification (tests/depth_stats_ref.py) against its brute-force restatement and
against hand cases whose sums are exact, the checker against planted faults, and the host side of the feature -- argument validation before
any launch, the ctypes rows, the ABI number."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import depth_stats_ref as R


@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("S", [1, 2, 7, 64, 65, 300])
def test_spec_equals_the_brute_force_restatement(S, closed):
    qs = (0.1, 0.5, 0.75, 0.95)
    for seed in range(3):
        w, z, dirs = R.make_inputs(11, S, closed, seed)
        for mul in (True, False):
            ref = R.spec(w, z, dirs, qs, 2.0, 6.0, mul)
            want, opacity = R.brute(w, z, dirs, qs, 2.0, 6.0, mul)
            # the same fp64 operations in the same order up to the association of the interpolation: a few ulps of fp64
            assert np.abs(ref["depth_q"] - want).max() <= 1e-13 * (1.0 + np.abs(want).max())
            assert np.array_equal(ref["opacity"], opacity)
        assert set(np.unique(ref["k"])) <= set(range(-1, S))


def test_hand_cases_with_exact_sums():
    z = np.array([[1.0, 2.0, 4.0, 8.0]], np.float32)                      # closed row of three intervals
    w = np.array([[0.25, 0.25, 0.5]], np.float32)
    r = R.spec(w, z, None, (0.5,))
    assert r["k"][0, 0] == 1 and r["D"][0, 0] == 4.0 and r["opacity"][0] == 1.0        # q = 1/2 lands exactly on t_2
    r = R.spec(w, z, None, (0.125, 0.75))
    assert r["D"][0].tolist() == [1.5, 6.0]
    d = np.array([[0.0, 3.0, 4.0]], np.float32)                           # |d| = 5
    r = R.spec(w, z, d, (0.75,), near=10.0, far=50.0)
    assert r["D"][0, 0] == 30.0 and r["depth_q"][0, 0] == 0.5
    assert R.spec(w, z, d, (0.75,), mul_norm=False)["D"][0, 0] == 6.0
    # an all-zero ray: the far edge, opacity 0 -- closed and open
    zero = np.zeros((1, 3), np.float32)
    r = R.spec(zero, z, None, (0.5,))
    assert r["k"][0, 0] == -1 and r["D"][0, 0] == 8.0 and r["opacity"][0] == 0.0
    assert R.spec(zero, z[:, :3], None, (0.5,))["D"][0, 0] == 4.0
    # total mass below q
    r = R.spec(np.array([[0.25, 0.125, 0.0]], np.float32), z, None, (0.25, 0.5))
    assert r["D"][0].tolist() == [2.0, 8.0] and r["opacity"][0] == 0.375
    # S = 1, closed and open
    one = np.array([[0.5]], np.float32)
    assert R.spec(one, np.array([[2.0, 6.0]], np.float32), None, (0.25, 0.5, 0.75))["D"][0].tolist() == [4.0, 6.0, 6.0]
    assert R.spec(one, np.array([[2.0]], np.float32), None, (0.25, 0.75))["D"][0].tolist() == [2.0, 2.0]
    # an open row whose crossing is the last sample returns that sample's depth; one before it interpolates
    r = R.spec(w, z[:, :3], None, (0.375, 0.75))
    assert r["D"][0].tolist() == [3.0, 4.0]
    # the brute force says the same
    got, op = R.brute(w, z, d, (0.125, 0.5, 0.75), near=10.0, far=50.0)
    assert got[0].tolist() == [(7.5 - 10.0) / 40.0, 0.25, 0.5] and op[0] == 1.0


def _as_fp32(ref):
    return ref["depth_q"].astype(np.float32), ref["opacity"].astype(np.float32)


def test_the_checker_passes_the_rounded_specification_and_excludes_nothing_on_the_test_inputs():
    """the device sweep's inputs: the specification alone reports ZERO pairs on an edge next to an empty interval"""
    total = 0
    for S in R.GPU_S:
        for closed in (True, False):
            for N in R.GPU_N:
                w, z, dirs = R.make_inputs(N, S, closed, S + N)
                qs = (0.1, 0.25, 0.5, 0.95)
                dq, op = _as_fp32(R.spec(w, z, dirs, qs, 2.0, 6.0))
                ratio, ulps, n_excl, n_pairs = R.check(dq, op, w, z, dirs, qs, 2.0, 6.0)
                assert n_excl == 0 and ratio <= 1.0 and ulps == 0.0, (S, closed, N, ratio, ulps, n_excl)
                total += n_pairs
    assert total == 4 * sum(R.GPU_N) * 2 * len(R.GPU_S)


def test_the_exclusion_is_the_edge_next_to_an_empty_interval_and_nothing_else():
    z = np.array([[1.0, 2.0, 4.0, 8.0]], np.float32)
    w = np.array([[0.5, 0.0, 0.5]], np.float32)                           # C reaches 1/2 exactly where an empty interval begins: D jumps from 2 to 4
    assert R.check(None, None, w, z, None, (0.5,))[2:] == (1, 1)
    assert R.check(None, None, w, z, None, (0.25, 0.75))[2:] == (0, 2)
    assert R.check(None, None, np.array([[0.25, 0.25, 0.5]], np.float32), z, None, (0.5,))[2:] == (0, 1)


FAULTS = {"fp32 cumsum": dict(cum_dtype=np.float32), "renormalised mass": dict(renormalise=True), "off-by-one edge": dict(edge_shift=1),
          "forgotten |d|": dict(use_norm=False)}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_the_checker_catches_planted_faults(fault):
    qs = (0.25, 0.5)
    w, z, dirs = R.make_inputs(40, 1087, True, 0)
    bad = R._evaluate(w, z, dirs, qs, 2.0, 6.0, True, **FAULTS[fault])
    ratio, _, n_excl, _ = R.check(bad["depth_q"].astype(np.float32), None, w, z, dirs, qs, 2.0, 6.0)
    good, _, _, _ = R.check(R.spec(w, z, dirs, qs, 2.0, 6.0)["depth_q"].astype(np.float32), None, w, z, dirs, qs, 2.0, 6.0)
    print("%s: worst err / tol %.3g (the rounded specification: %.3g)" % (fault, ratio, good))
    assert n_excl == 0 and good <= 1.0 and ratio > 1.0
    if fault == "fp32 cumsum":                                          # opacity too: an fp32 running sum of 1087 terms is not within an ulp
        assert R.check(None, bad["opacity"].astype(np.float32), w, z, dirs, qs)[1] > 1.0


# ------------------------------------------------------------------------------------------------ the host side of the package
def test_abi_number_and_signature_rows():
    from nerf_amd import _lib
    assert _lib.lib.nerf_amd_version() == 125 and _lib.EXPECTED_VERSION == 125
    assert _lib.DEPTH_QUANTILES_MAX == R.QUANTILES_MAX == 4
    res, args = _lib.SIGNATURES["nerf_amd_ray_depth_stats"]
    assert res is ctypes.c_int and len(args) == 16
    assert _lib.SIGNATURES["nerf_amd_render"] == (ctypes.c_int, [ctypes.POINTER(_lib.RenderRequest), ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES["nerf_amd_render_request_workspace_bytes"] == (ctypes.c_size_t, [ctypes.POINTER(_lib.RenderRequest)])
    for name in ("nerf_amd_ray_depth_stats", "nerf_amd_render", "nerf_amd_render_request_workspace_bytes"):
        assert name in _lib.ADDED_AFTER_125 and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # the descriptor of samples keeps its layout
    assert ctypes.sizeof(_lib.Samples) == 168


def test_request_mirror_and_workspace_queries():
    """the struct mirror is the library's layout: a request with no new output sizes its workspace exactly like the entry point it stands
    for, and only the request's own query grows with the new outputs"""
    from nerf_amd import _lib
    lib = _lib.lib
    r = _lib.RenderRequest(N=1000, n_fine=128)
    assert r.size == ctypes.sizeof(_lib.RenderRequest) and r.size % 8 == 0
    q = lambda: lib.nerf_amd_render_request_workspace_bytes(ctypes.byref(r))
    assert q() == lib.nerf_amd_render_workspace_bytes(1000, 128) > 0
    r.spacing = _lib.SPACING_DISPARITY
    r.near, r.far = 0.2, 100.0
    assert q() == lib.nerf_amd_render_warped_workspace_bytes(1000, 128)
    r.prop_pnum = 64
    assert q() == lib.nerf_amd_render_rounds_workspace_bytes(1000, 128, 64, _lib.SPACING_DISPARITY)
    r.spacing, r.prop_pnum, r.ref = _lib.SPACING_LINEAR, 0, 1
    base = lib.nerf_amd_render_ref_workspace_bytes(1000, 128)
    assert q() == base
    r.fine_depths = 8                                                    # (an address is all the query looks at) a copy needs no scratch
    assert q() == base
    r.opacity = 8                                                        # the weights the stats kernel reads: (N, n_fine + 64), appended
    assert q() >= base + 1000 * 192 * 4 and q() <= base + 1000 * 192 * 4 + 1024
    r.weights = 8                                                        # ... unless the caller takes them
    assert q() == base
    # refusals, all before any launch
    r.size = 8
    assert q() == 0 and lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"size" in lib.nerf_amd_last_error()
    r.size = ctypes.sizeof(_lib.RenderRequest)
    r.n_quantiles = 5
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"n_quantiles" in lib.nerf_amd_last_error()
    r.n_quantiles = 1
    r.quantiles[0] = 1.0
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"(0, 1)" in lib.nerf_amd_last_error()
    r.quantiles[0] = 0.5
    r.spacing = 7
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"spacing" in lib.nerf_amd_last_error()
    r.spacing, r.prop_pnum = _lib.SPACING_LINEAR, 64
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -2       # Ref-NeRF has no second round
    assert lib.nerf_amd_render(None, None, None) == -1


def test_stats_entry_point_refusals_before_any_launch():
    from nerf_amd import _lib
    lib = _lib.lib
    q = (ctypes.c_float * 4)(0.5, 0.25, 0.75, 0.9)
    p = ctypes.c_void_p(256)                                             # never dereferenced: every call below is refused on the host
    def call(**kw):
        a = dict(w=p, z=p, zs=9, closed=1, d=p, ds=3, N=4, S=8, mul=1, q=q, nq=1, near=0.0, far=1.0, op=p, dq=p, st=None)
        a.update(kw)
        return lib.nerf_amd_ray_depth_stats(*[a[k] for k in ("w", "z", "zs", "closed", "d", "ds", "N", "S", "mul", "q", "nq", "near", "far", "op", "dq", "st")])

    assert call(N=0) == 0                                                # nothing to do is not an error
    for bad in (dict(N=-1), dict(S=0), dict(nq=5), dict(nq=-1), dict(zs=8), dict(w=None), dict(z=None), dict(d=None), dict(dq=None), dict(q=None),
                dict(q=(ctypes.c_float * 1)(0.0)), dict(q=(ctypes.c_float * 1)(1.0)), dict(q=(ctypes.c_float * 1)(float("nan"))), dict(ds=2)):
        assert call(**bad) == -1, bad
    assert call(zs=8, closed=0, N=0) == 0 and call(d=None, mul=0, N=0) == 0


def test_python_argument_errors_are_value_errors_on_the_host():
    from nerf_amd import ops, parallel, procedures
    w, z = torch.zeros(3, 8), torch.zeros(3, 9)                          # CPU tensors: a ValueError must come before the device check
    for bad in ((0.0,), (1.0,), (float("nan"),), (0.1, 0.2, 0.3, 0.4, 0.5), ("a",), (-0.5,)):
        with pytest.raises(ValueError):
            ops.ray_depth_stats(w, z, quantiles=bad)
        with pytest.raises(ValueError):
            procedures.render_image(None, None, torch.zeros(3, 4), 8, 10.0, 2.0, 6.0, depth_quantiles=bad)
        for fn in (ops.render_rays, ops.render_rays_ref):
            with pytest.raises(ValueError):
                fn(None, None, 0, None, None, None, None, 8, 2.0, 6.0, True, quantiles=bad)
        with pytest.raises(ValueError):
            ops.render_rays_warped(None, None, 0, None, None, None, 8, 2.0, 6.0, True, quantiles=bad)
        with pytest.raises(ValueError):
            ops.render_rays_rounds(None, None, 0, None, None, 8, 2.0, 6.0, True, prop_pnum=16, seed=0, quantiles=bad)
    # what the argument-list C entry points refused by being the one called: the request reads prop_pnum = 0 as one round and linear spacing
    # as the plain pipeline, so the package refuses both itself, before any tensor is touched, with and without the optional outputs
    for kw in (dict(), dict(quantiles=(0.5,))):
        for p in (0, 2, 257):
            with pytest.raises(ValueError, match="prop_pnum"):
                ops.render_rays_rounds(None, None, 0, None, None, 8, 2.0, 6.0, True, prop_pnum=p, seed=0, **kw)
        with pytest.raises(ValueError, match="spacing"):
            ops.render_rays_warped(None, None, 0, None, None, None, 8, 2.0, 6.0, True, spacing="linear", **kw)
    for bad_w, bad_z in ((torch.zeros(3, 8), torch.zeros(3, 10)), (torch.zeros(3, 8), torch.zeros(4, 9)), (torch.zeros(3, 0), torch.zeros(3, 1)),
                         (torch.zeros(8), torch.zeros(9))):
        with pytest.raises(ValueError):
            ops.ray_depth_stats(bad_w, bad_z)
    with pytest.raises(ValueError):
        ops.ray_depth_stats(w, z, torch.zeros(3, 4))
    assert ops.depth_quantiles(None) == () and ops.depth_quantiles(0.5) == (0.5,) and ops.depth_quantiles([0.25, 0.5]) == (0.25, 0.5)
    # appended, keyword-only, off by default
    assert not hasattr(ops, "render_rays_rounds_stats")                  # (one function per pipeline: the twin is gone)
    for fn in (ops.render_rays, ops.render_rays_warped, ops.render_rays_rounds, ops.render_rays_ref):
        p = inspect.signature(fn).parameters
        assert [(n, p[n].default, p[n].kind) for n in list(p)[-3:]] == [("quantiles", None, inspect.Parameter.KEYWORD_ONLY),
                                                                        ("want_opacity", False, inspect.Parameter.KEYWORD_ONLY),
                                                                        ("want_fine_depths", False, inspect.Parameter.KEYWORD_ONLY)], fn
    for fn in (procedures.render_image, parallel.render_image_sharded, procedures._render_rays_by_calls):
        p = inspect.signature(fn).parameters
        assert [(n, p[n].default, p[n].kind) for n in list(p)[-2:]] == [("depth_quantiles", None, inspect.Parameter.KEYWORD_ONLY),
                                                                        ("render_opacity", False, inspect.Parameter.KEYWORD_ONLY)], fn
    p = inspect.signature(ops.ray_depth_stats).parameters
    assert list(p)[:3] == ["weights", "z", "dirs"] and all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[3:])
    assert p["quantiles"].default == (0.5,) and p["mul_norm"].default is True and p["want_opacity"].default is True
    for fn in (ops.ray_depth_stats, procedures.render_image):
        assert "ABSOLUTE" in fn.__doc__ and "far edge" in fn.__doc__
