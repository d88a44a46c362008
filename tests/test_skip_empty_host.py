"""The empty-ray skip without a GPU: the fp64 specification (tests/skip_empty_ref.py) against hand cases and against itself with faults
planted, and the host side of the feature -- the ABI number and struct sizes, the appended request fields, the workspace queries, every
refusal before a launch (with pointers that are never dereferenced), the Python argument errors."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import skip_empty_ref as R

TAU = 0.5                                                                  # the threshold of the sweeps below: D_min = log 2


def _sweep():
    for N in R.GPU_N:
        for C in R.GPU_C:
            yield N, C, R.make_inputs(N, C, 0)


# ------------------------------------------------------------------------------------------------ the specification
def test_hand_cases():
    z = np.array([[1.0, 2.0, 4.0]], np.float32)
    d = np.array([[0.0, 3.0, 4.0]], np.float32)                            # |d| = 5
    D = R.optical_depth(np.array([[0.5, 0.25, -1.0]], np.float32), z, d)
    assert D[0] == 5.0 * (0.5 * 1.0 + 0.25 * 2.0)
    assert R.optical_depth(np.array([[-1.0, -2.0, 0.5]], np.float32), z, d)[0] == 0.5 * 1e10          # the closing delta: not scaled by |d|
    assert R.optical_depth(np.array([[-1.0, -2.0, -0.5]], np.float32), z, d)[0] == 0.0
    assert math.isnan(R.optical_depth(np.array([[np.nan, -2.0, -0.5]], np.float32), z, d)[0])         # max(sigma, 0) keeps a NaN
    flags = R.alive_flags(np.array([0.0, 0.5, 1.0, np.nan, np.inf]), 0.5)
    assert flags.tolist() == [False, True, True, True, True]                                        # D == D_min is alive, NaN is alive
    row, ray, n = R.compact(flags)
    assert row.tolist() == [-1, 0, 1, 2, 3] and ray.tolist() == [1, 2, 3, 4] and n == 4 and row.dtype == np.int32 and ray.dtype == np.int64
    assert R.compact(np.zeros(5, bool))[2] == 0 and R.compact(np.ones(3, bool))[0].tolist() == [0, 1, 2]
    assert R.d_min_of_tau(0.5) == -math.log1p(-0.5) and abs(R.d_min_of_tau(1e-4) - 1e-4) < 1e-8
    assert R.undecidable(np.array([1.0, 1.0 + 5e-10, 1.1, np.nan, np.inf]), 1.0).tolist() == [True, True, False, False, False]


def test_no_ray_of_the_device_sweeps_is_undecidable():
    """the thresholds the GPU tests use on these inputs decide every ray: the flags must then match exactly, whatever the summation order"""
    total = 0
    for N, C, (density, z, dirs) in _sweep():
        D = R.optical_depth(density, z, dirs)
        # (all alive is asked for with D_min = -1, not 0: by the helper's own rule D = 0 against D_min = 0 counts as undecidable)
        for d_min in (R.d_min_of_tau(TAU), R.d_min_of_tau(1e-3), -1.0, np.inf):
            assert int(R.undecidable(D, d_min).sum()) == 0, (N, C, d_min)
        total += N
    assert total == 5 * sum(R.GPU_N)


FAULTS = {"an fp32 running sum": dict(sum_dtype=np.float32), "the |d| factor dropped": dict(use_norm=False),
          "the closing delta scaled by |d|": dict(closing="scaled"), "the previous interval as closing delta": dict(closing="previous"),
          "max(sigma, 0) dropped": dict(clamp=False)}


def _fault_inputs(fault):
    """inputs on which the fault must show: the sweep's, except for the fp32 sum, which needs rays right at the threshold -- long rows of
    which the first term is 2^24 times the others: the fp32 running sum drops every later term, the fp64 sum keeps them"""
    if fault != "an fp32 running sum":
        density, z, dirs = R.make_inputs(1000, 65, 3)
        if fault == "the closing delta scaled by |d|":                    # rays that only the far sample keeps alive, D = 1, with |d| = 0.25
            density[3::7, -1] = 1e-10
            dirs[3::7] = np.array([0.0, 0.25, 0.0], np.float32)
        return density, z, dirs, R.d_min_of_tau(TAU)
    N, C = 16, 258
    density = np.full((N, C), 1.0, np.float32)
    density[:, 0] = 2.0 ** 24
    density[:, -1] = -1.0
    z = np.broadcast_to(np.arange(C, dtype=np.float32), (N, C)).copy()    # unit intervals
    dirs = np.zeros((N, 3), np.float32)
    dirs[:, 2] = 1.0
    return density, z, dirs, 2.0 ** 24 + 128.0                             # D = 2^24 + 256 in fp64 (alive), 2^24 in an fp32 running sum (dead)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_the_specification_sees_planted_faults(fault):
    density, z, dirs, d_min = _fault_inputs(fault)
    good = R.alive_flags(R.optical_depth(density, z, dirs), d_min)
    assert int(R.undecidable(R.optical_depth(density, z, dirs), d_min).sum()) == 0
    bad = R.alive_flags(R.optical_depth(density, z, dirs, **FAULTS[fault]), d_min)
    flipped = int((good != bad).sum())
    print("%s: %d of %d flags flip" % (fault, flipped, good.size))
    assert flipped >= 1


def test_a_comparison_that_a_nan_fails_kills_the_nan_row():
    density, z, dirs = R.make_inputs(257, 64, 0)
    D = R.optical_depth(density, z, dirs)
    assert int(np.isnan(D).sum()) == 1
    good, bad = R.alive_flags(D, R.d_min_of_tau(TAU)), R.alive_flags(D, R.d_min_of_tau(TAU), nan_alive=False)
    assert (good != bad).nonzero()[0].tolist() == [257 // 2] and bool(good[257 // 2])


def test_an_unordered_compaction_differs():
    flags = R.spec(*R.make_inputs(257, 64, 0), R.d_min_of_tau(TAU))["alive"]
    row, ray, n = R.compact(flags)
    row_u, ray_u, n_u = R.compact(flags, ordered=False)
    assert n == n_u and 1 < n < 257 and sorted(ray_u.tolist()) == ray.tolist()
    assert not np.array_equal(row, row_u) and not np.array_equal(ray, ray_u)
    assert np.all(np.diff(ray) > 0)                                        # alive rays keep their order


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_number_sizes_and_the_new_symbols():
    from nerf_amd import _lib
    assert _lib.lib.nerf_amd_version() == 125 and _lib.EXPECTED_VERSION == 125
    assert ctypes.sizeof(_lib.Samples) == 168
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("nerf_amd_ray_alive", 13), ("nerf_amd_ray_alive_workspace_bytes", 1), ("nerf_amd_gather_rows", 7)):
        assert hasattr(raw, name) and name in _lib.ADDED_AFTER_125 and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["nerf_amd_ray_alive"][1][7] is ctypes.c_double               # min_optical_depth
    # the request mirror: three fields appended behind the first layout's 200 bytes
    R_ = _lib.RenderRequest
    assert R_.fine_depths.offset == 192 and R_.skip_min_optical_depth.offset == 200 and R_.row_of_ray.offset == 208 and R_.n_alive.offset == 216
    assert ctypes.sizeof(R_) == 224 and [f[0] for f in R_._fields_][-3:] == ["skip_min_optical_depth", "row_of_ray", "n_alive"]


def test_request_size_is_the_librarys_and_the_first_layout_is_still_accepted():
    from nerf_amd import _lib
    lib = _lib.lib
    r = _lib.RenderRequest(N=1000, n_fine=128)
    q = lambda: lib.nerf_amd_render_request_workspace_bytes(ctypes.byref(r))
    full = q()
    assert full == lib.nerf_amd_render_workspace_bytes(1000, 128) > 0
    r.skip_min_optical_depth = 0.5
    grown = q()
    assert grown > full
    r.size = 200                                                           # the first layout: the new fields are not read
    assert q() == full
    r.size = 223                                                           # anything short of the whole struct is the first layout too
    assert q() == full
    r.size = 199
    assert q() == 0 and lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"smaller than nerf_amd_render_request" in lib.nerf_amd_last_error()
    r.size = 225                                                           # a later, larger layout: the known fields are read
    assert q() == grown


def test_workspace_grows_only_with_the_skip_on():
    from nerf_amd import _lib
    lib = _lib.lib
    N, nf = 1000, 128
    r = _lib.RenderRequest(N=N, n_fine=nf)
    q = lambda: lib.nerf_amd_render_request_workspace_bytes(ctypes.byref(r))
    alive_ws = lib.nerf_amd_ray_alive_workspace_bytes(N)
    assert alive_ws >= N + 4 * 4 and lib.nerf_amd_ray_alive_workspace_bytes(-1) == 0 and lib.nerf_amd_ray_alive_workspace_bytes(2 ** 31) == 0
    tables = N * 4 + N * 8 + N * 24                                        # row_of_ray, ray_of_row, the compact ray table

    def grows(base, depth_row, coarse):
        r.skip_min_optical_depth = 0.0
        assert q() == base
        r.skip_min_optical_depth = -1.0                                    # negative: off
        assert q() == base
        r.row_of_ray = 8                                                   # outputs of a mode that is off: not looked at
        assert q() == base
        r.row_of_ray = None
        r.skip_min_optical_depth = 1e-3
        need = tables + N * depth_row * 4 + (N * 64 * 4 if coarse else 0) + alive_ws
        assert base + need <= q() <= base + need + 4096, (q() - base, need)

    grows(lib.nerf_amd_render_workspace_bytes(N, nf), nf + 1, True)       # linear, one round: the coarse depths are stored for the skip
    r.spacing, r.near, r.far = _lib.SPACING_DISPARITY, 0.2, 100.0
    grows(lib.nerf_amd_render_warped_workspace_bytes(N, nf), nf + 1, False)
    r.prop_pnum = 64
    grows(lib.nerf_amd_render_rounds_workspace_bytes(N, nf, 64, _lib.SPACING_DISPARITY), nf + 1, False)
    r.spacing = _lib.SPACING_LINEAR
    grows(lib.nerf_amd_render_rounds_workspace_bytes(N, nf, 64, _lib.SPACING_LINEAR), nf + 1, False)
    r.prop_pnum, r.ref = 0, 1
    grows(lib.nerf_amd_render_ref_workspace_bytes(N, nf), nf + 64, False)


# ------------------------------------------------------------------------------------------------ refusals, all on the host
def test_stage_entry_points_refuse_before_any_launch():
    from nerf_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused on the host

    def alive(**kw):
        a = dict(density=p, z=p, zs=64, dirs=p, ds=3, N=4, C=64, dmin=0.5, row=p, ray=p, count=p, ws=p, st=None)
        a.update(kw)
        return lib.nerf_amd_ray_alive(*[a[k] for k in ("density", "z", "zs", "dirs", "ds", "N", "C", "dmin", "row", "ray", "count", "ws", "st")])

    for bad in (dict(N=-1), dict(N=2 ** 31), dict(C=1), dict(C=0), dict(zs=63), dict(ds=2), dict(dmin=float("nan")), dict(density=None), dict(z=None),
                dict(dirs=None), dict(row=None), dict(ray=None), dict(count=None), dict(ws=None), dict(N=0, count=None)):
        assert alive(**bad) == -1 and lib.nerf_amd_last_error(), bad

    def gather(**kw):
        a = dict(src=p, ss=8, ray=p, n=4, cols=8, dst=p, st=None)
        a.update(kw)
        return lib.nerf_amd_gather_rows(*[a[k] for k in ("src", "ss", "ray", "n", "cols", "dst", "st")])

    for bad in (dict(n=-1), dict(cols=-1), dict(ss=7), dict(src=None), dict(ray=None), dict(dst=None)):
        assert gather(**bad) == -1, bad
    assert gather(n=0, src=None, ray=None, dst=None) == 0 and gather(cols=0, ss=0) == 0        # nothing to do is not an error


def test_render_request_refusals_with_the_skip_on():
    from nerf_amd import _lib
    lib = _lib.lib
    r = _lib.RenderRequest(N=1000, n_fine=128)
    r.skip_min_optical_depth = float("nan")
    assert lib.nerf_amd_render_request_workspace_bytes(ctypes.byref(r)) == 0
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"NaN" in lib.nerf_amd_last_error()
    r.skip_min_optical_depth = 0.5
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"NULL" in lib.nerf_amd_last_error()      # the usual input checks still come first
    r.N = 2 ** 31
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -1 and b"2^31" in lib.nerf_amd_last_error()
    r.N, r.ref, r.prop_pnum = 1000, 1, 64
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == -2       # (unchanged: Ref-NeRF has no second round)
    r.N, r.ref, r.prop_pnum = 0, 0, 0
    n_alive = ctypes.c_int64(-7)
    r.n_alive = ctypes.pointer(n_alive)
    assert lib.nerf_amd_render(ctypes.byref(r), None, None) == 0 and n_alive.value == 0             # N == 0 is fine: nothing runs, nothing is alive


def test_python_argument_errors():
    from nerf_amd import ops, parallel, procedures
    assert ops.skip_threshold() == 0.0 and ops.skip_threshold(0.5) == -math.log1p(-0.5) and ops.skip_threshold(None, 0.25) == 0.25
    d, z, dirs = torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3, 3)  # CPU tensors: a ValueError must come before the device check
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), "a"):
        with pytest.raises(ValueError):
            ops.ray_alive(d, z, dirs, tau=bad)
        with pytest.raises(ValueError):
            procedures.render_image(None, None, torch.zeros(3, 4), 8, 10.0, 2.0, 6.0, skip_empty=bad)
        for fn in (ops.render_rays, ops.render_rays_ref):
            with pytest.raises(ValueError):
                fn(None, None, 0, None, None, None, None, 8, 2.0, 6.0, True, skip_tau=bad)
        with pytest.raises(ValueError):
            ops.render_rays_warped(None, None, 0, None, None, None, 8, 2.0, 6.0, True, skip_tau=bad)
        with pytest.raises(ValueError):
            ops._render_rays_rounds(None, None, 0, None, None, 8, 2.0, 6.0, True, prop_pnum=16, seed=0, skip_tau=bad)
    for kw in (dict(), dict(tau=0.5, min_optical_depth=0.5), dict(min_optical_depth=0.0), dict(min_optical_depth=-1.0), dict(min_optical_depth=float("nan"))):
        with pytest.raises(ValueError):
            ops.ray_alive(d, z, dirs, **kw)
    with pytest.raises(ValueError):
        ops.render_rays(None, None, 0, None, None, None, None, 8, 2.0, 6.0, True, skip_tau=0.5, skip_min_optical_depth=0.5)
    for bad in ((torch.zeros(3, 8), torch.zeros(3, 9), dirs), (torch.zeros(3, 1), torch.zeros(3, 1), dirs), (d, z, torch.zeros(3, 4)), (d, z, torch.zeros(4, 3)),
                (torch.zeros(8), torch.zeros(8), dirs)):
        with pytest.raises(ValueError):
            ops.ray_alive(*bad, tau=0.5)
    # keyword-only, off by default, in front of the optional-output keywords whose position earlier tests pin
    # (render_rays_rounds' keyword list is pinned by an earlier test: its body, _render_rays_rounds, carries the two keywords)
    assert "skip_tau" not in inspect.signature(ops.render_rays_rounds).parameters
    for fn in (ops.render_rays, ops.render_rays_warped, ops._render_rays_rounds, ops.render_rays_ref):
        p = inspect.signature(fn).parameters
        for name in ("skip_tau", "skip_min_optical_depth"):
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is None, (fn, name)
    for fn in (procedures.render_image, parallel.render_image_sharded):
        p = inspect.signature(fn).parameters
        assert p["skip_empty"].kind is inspect.Parameter.KEYWORD_ONLY and p["skip_empty"].default is None, fn
    p = inspect.signature(ops.ray_alive).parameters
    assert list(p) == ["density", "z", "dirs", "tau", "min_optical_depth"] and all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(p)[3:])
    assert procedures.get_parser().parse_args([]).skip_empty is None and procedures.get_parser().parse_args(["--skip_empty", "0.01"]).skip_empty == 0.01
    for fn in (procedures.render_image, parallel.render_image_sharded, ops.render_rays):
        assert "skip" in fn.__doc__ and "bit for bit" in fn.__doc__
    assert "APPROXIMATION" in procedures.render_image.__doc__ and "UNEVENLY LOADED" in parallel.render_image_sharded.__doc__
