"""The two-round render entry point, host side (no GPU): the two symbols are declared, bound and exported under the unchanged ABI number, the
workspace query is monotone and covers the parts the header lists, every argument check answers before any HIP call, and the op has the
signature render_image relies on."""
import ctypes as C
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nerf_amd_render_rounds_workspace_bytes", "nerf_amd_render_rays_rounds")
LINEAR, DISPARITY = 0, 1


def test_symbols_are_declared_bound_and_the_abi_number_stays():
    from nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert "size_t nerf_amd_render_rounds_workspace_bytes(int64_t N, int n_fine, int prop_pnum, int spacing);" in header
    assert "int    nerf_amd_render_rays_rounds(" in header
    for name in NAMES:
        assert name in _lib.SIGNATURES and name in _lib.ADDED_AFTER_125 and hasattr(_lib.lib, name), name
    assert len(_lib.SIGNATURES["nerf_amd_render_rays_rounds"][1]) == 19
    assert _lib.lib.nerf_amd_version() == 125 and _lib.EXPECTED_VERSION == 125


def _parts(N, nf, P, spacing):
    """the workspace parts of the header comment, unrounded"""
    floats = N * 64 + 2 * N * P + N * (nf + 1) + N * nf * 4 + N * 6
    if spacing == DISPARITY:
        floats += 2 * N * 64 + N * P + N
    return 4 * floats


@pytest.mark.parametrize("spacing", [LINEAR, DISPARITY])
def test_workspace_query(spacing):
    from nerf_amd import _lib
    q = _lib.lib.nerf_amd_render_rounds_workspace_bytes
    for N, nf, P in ((1, 1, 3), (5, 64, 48), (1600, 128, 64), (640000, 128, 64), (333, 1023, 256)):
        got = q(N, nf, P, spacing)
        assert got >= _parts(N, nf, P, spacing) > 0, (N, nf, P)
        assert got <= _parts(N, nf, P, spacing) + 16 * 256 + 512, (N, nf, P)           # at most one rounding per part and the slack
    base = q(1000, 128, 64, spacing)
    assert q(1001, 128, 64, spacing) > base and q(1000, 129, 64, spacing) > base and q(1000, 128, 65, spacing) > base
    for a, b in zip(range(0, 300, 7), range(7, 307, 7)):
        assert q(a, 128, 64, spacing) <= q(b, 128, 64, spacing)
        assert q(100, max(a, 1), 64, spacing) <= q(100, b, 64, spacing)
    for a in range(3, 256):
        assert q(100, 128, a, spacing) <= q(100, 128, a + 1, spacing)
    assert q(100, 128, 64, DISPARITY) > q(100, 128, 64, LINEAR)
    for bad in ((-1, 128, 64, spacing), (10, 0, 64, spacing), (10, 1024, 64, spacing), (10, 128, 2, spacing), (10, 128, 257, spacing), (10, 128, 64, 2),
                (10, 128, 64, -1)):
        assert q(*bad) == 0, bad


def _call():
    """(lib, the argument list of a call that passes every check -- on HOST memory: a call that got past the checks would fail in HIP)"""
    from nerf_amd import _lib
    bufs = [(C.c_float * 64)() for _ in range(7)]
    prop, mip, rays, z_base, rgb, depth, ws = (C.cast(b, C.c_void_p) for b in bufs)
    cam = _lib.Samples()
    # packed_prop packed_mip precision rays camera ray_offset z_base N n_fine prop_pnum spacing near far white_bkg rgb depth weights workspace stream
    return _lib, [prop, mip, _lib.F32, rays, C.byref(cam), 0, z_base, 4, 64, 48, LINEAR, 2.0, 6.0, 1, rgb, depth, None, ws, None], cam


def test_abi_validates_before_any_hip_call():
    _lib, full, cam = _call()
    lib = _lib.lib
    fn = lib.nerf_amd_render_rays_rounds
    PREC, RAYS, CAM, ZBASE, N, NF, P, SPACING, NEAR, FAR, RGB, WS = 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14, 17

    def refused(changes, needle=None):
        a = list(full)
        for k, v in changes.items():
            a[k] = v
        assert fn(*a) == -1, changes
        msg = lib.nerf_amd_last_error()
        assert msg, changes
        if needle:
            assert needle in msg, (changes, msg)

    for p in (2, 256 + 1, 0, -5):
        refused({P: p}, b"prop_pnum")
    for nf in (0, 1024, -1):
        refused({NF: nf}, b"n_fine")
    refused({N: -1})
    refused({P: 256, NF: 1023}, b"LDS")                                                  # linear: 16 (5 * 256 + 3 * 1024 + 1280) bytes > 64 KiB
    refused({P: 256, NF: 1023, SPACING: DISPARITY, NEAR: 0.2, FAR: 1000.0}, b"LDS")
    refused({P: 64, NF: 800, SPACING: DISPARITY, NEAR: 0.2, FAR: 1000.0}, b"LDS")         # 16 (320 + 4 * 801 + 1280) > 64 KiB where linear's 3 K still fits
    assert _lib.lib.nerf_amd_render_rounds_workspace_bytes(4, 800, 64, LINEAR) > 0
    for prec in (7, -1, _lib.F32 | 0x400, _lib.BF16_F8):
        refused({PREC: prec}, b"precision")
    cam.ipe, cam.ipe_radius = 1, 0.01
    refused({PREC: _lib.BF16 | _lib.FINE_W128}, b"128-wide")
    refused({SPACING: DISPARITY, NEAR: 0.2, FAR: 1000.0, RAYS: None}, b"ray table")       # IPE under disparity spacing: explicit rays
    cam.ipe, cam.ipe_radius = 1, 0.0
    refused({}, b"ipe_radius")
    cam.ipe, cam.ipe_radius = 0, 0.0
    for spacing in (2, -1, 7):
        refused({SPACING: spacing}, b"spacing")
    refused({SPACING: DISPARITY, NEAR: 0.0, FAR: 6.0}, b"near")
    refused({SPACING: DISPARITY, NEAR: 2.0, FAR: 2.0}, b"far")
    for hole in (0, 1, CAM, ZBASE, RGB, WS):
        refused({hole: None}, b"NULL")
    refused({SPACING: DISPARITY, NEAR: 0.2, FAR: 1000.0, ZBASE: None, RGB: None}, b"NULL")   # z_base is not read under disparity spacing: rgb is what is missing
    refused({RAYS: None}, b"camera image")                                               # no ray table and no camera image to generate one from
    a = list(full)
    a[N] = 0
    assert fn(*a) == 0                                                                   # nothing to do, nothing launched


def test_op_signature():
    from nerf_amd import ops
    p = inspect.signature(ops.render_rays_rounds).parameters
    assert list(p)[:9] == ["packed_prop", "packed_mip", "precision", "rays", "z_base", "n_fine", "near", "far", "white_bkg"]
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in list(p)[:9])
    keyword_only = dict(prop_pnum=inspect.Parameter.empty, seed=inspect.Parameter.empty, rng_ray_offset=0, spacing="linear", contract=False, ipe_radius=None,
                        ipe_dir_norm=None, want_depth=True, want_weights=False, workspace=None)
    assert list(p)[9:] == list(keyword_only) + ["quantiles", "want_opacity", "want_fine_depths"]       # the optional outputs, as in its three siblings
    keyword_only.update(quantiles=None, want_opacity=False, want_fine_depths=False)
    for name, default in keyword_only.items():
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    assert (ops.ROUNDS_PNUM_MIN, ops.ROUNDS_PNUM_MAX) == (3, 256)
