"""Disparity ray spacing, CPU side: the new C entry points exist and validate their arguments before any HIP call, the specification
(tests/ray_warp_ref.py) has the properties the design relies on, and the Python surface takes `spacing` keyword-only with "linear" as the
default."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import ray_warp_ref as R

PAIRS = ((2.0, 6.0), (0.2, 1000.0), (0.05, 1e6), (0.5, 64.0))
EPS = 2.0 ** -24


def test_warped_entry_points_validate_before_any_hip_call():
    from nerf_amd import _lib
    lib = _lib.lib
    D, L = _lib.SPACING_DISPARITY, _lib.SPACING_LINEAR
    p = ctypes.c_void_p(256)                                   # a non-NULL pointer nothing may dereference: every call below must fail first
    cases = []                                                 # (what, near, far, spacing, C)
    for what, near, far, spacing, Cn in (("near <= 0", 0.0, 6.0, D, 64), ("near < 0", -1.0, 6.0, D, 64), ("far <= near", 2.0, 2.0, D, 64),
                                         ("far < near", 2.0, 1.0, D, 64), ("linear is not a warped kind", 2.0, 6.0, L, 64),
                                         ("unknown spacing", 2.0, 6.0, 7, 64), ("C < 3", 2.0, 6.0, D, 2)):
        cases.append((what, near, far, spacing, Cn))
    for what, near, far, spacing, Cn in cases:
        if Cn >= 3:                                            # (C is no argument of these two)
            assert lib.nerf_amd_warp_depths(p, None, 4, 8, 0, spacing, near, far, p, None, None) == -1, what
            assert lib.nerf_amd_last_error()
            assert lib.nerf_amd_render_rays_warped(p, p, _lib.F32, p, None, 0, p, p, 4, 128, spacing, near, far, 0, p, None, None, p, None) == -1, what
        assert lib.nerf_amd_warped_stratified(p, p, 4, Cn, 0, 0, spacing, near, far, p, p, None, None) == -1, what
        assert lib.nerf_amd_warped_resample(p, p, p, 6, p, 4, Cn, 65, 0, 0.01, spacing, near, far, 0, 0, p, None, None, None, None) == -1, what
        assert lib.nerf_amd_last_error()
    # sizes and NULL pointers
    assert lib.nerf_amd_warp_depths(p, None, 4, 0, 0, D, 2.0, 6.0, p, None, None) == -1                       # S >= 1
    assert lib.nerf_amd_warp_depths(None, None, 4, 8, 0, D, 2.0, 6.0, p, None, None) == -1
    assert lib.nerf_amd_warp_depths(p, None, 4, 8, 0, D, 2.0, 6.0, p, p, None) == -1                          # pts without rays
    assert lib.nerf_amd_warped_stratified(p, p, 4, 257, 0, 0, D, 2.0, 6.0, p, p, None, None) == -1
    assert lib.nerf_amd_warped_stratified(p, None, 4, 130, 0, 0, D, 2.0, 6.0, p, p, None, None) == -1          # in-kernel Philox: 64 slots per ray
    assert lib.nerf_amd_warped_resample(p, p, p, 6, p, 4, 256, 1024, 0, 0.01, D, 2.0, 6.0, 0, 0, p, None, None, None, None) == -1   # LDS
    assert b"LDS" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_warped_resample(p, p, p, 6, p, 4, 64, 0, 0, 0.01, D, 2.0, 6.0, 0, 0, p, None, None, None, None) == -1
    assert lib.nerf_amd_warped_resample(p, p, None, 6, p, 4, 64, 65, 0, 0.01, D, 2.0, 6.0, 0, 0, p, None, None, None, None) == -1
    assert lib.nerf_amd_render_rays_warped(p, p, _lib.F32, p, None, 0, p, None, 4, 128, D, 2.0, 6.0, 0, p, None, None, p, None) == -1   # one of u_strat / u_inv
    assert lib.nerf_amd_render_rays_warped(p, p, _lib.F32, p, None, 0, None, None, 4, 128, D, 2.0, 6.0, 0, p, None, None, p, None) == -1  # Philox without descriptor
    assert lib.nerf_amd_render_rays_warped(p, p, 9, p, None, 0, p, p, 4, 128, D, 2.0, 6.0, 0, p, None, None, p, None) == -1
    # empty problems are fine and launch nothing
    assert lib.nerf_amd_warp_depths(None, None, 0, 8, 0, D, 2.0, 6.0, None, None, None) == 0
    assert lib.nerf_amd_render_rays_warped(None, None, _lib.F32, None, None, 0, None, None, 0, 128, D, 2.0, 6.0, 0, None, None, None, None, None) == 0
    assert lib.nerf_amd_render_warped_workspace_bytes(1000, 128) >= 1000 * (3 * 64 * 4 + 129 * 4 + 128 * 16 + 4 + 24)
    assert lib.nerf_amd_render_warped_workspace_bytes(-1, 128) == 0
    assert lib.nerf_amd_version() == 125                      # additive: the ABI number does not move


def test_spec_warp_end_points_monotone_and_inverse():
    for near, far in PAIRS:
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        ends = R.warp(torch.tensor([0.0, 1.0, -3.0, 7.0]), near, far)
        ulp_n, ulp_f = float(np.spacing(np.float32(near))), float(np.spacing(np.float32(far)))
        assert abs(float(ends[0]) - float(f32(near))) <= 2 * ulp_n and abs(float(ends[1]) - float(f32(far))) <= 2 * ulp_f
        assert float(ends[2]) == float(ends[0]) and float(ends[3]) == float(ends[1])                      # clamped
        s64 = torch.linspace(0.0, 1.0, 100001, dtype=torch.float64)
        z64 = R.warp(s64, near, far)
        assert bool((z64[1:] > z64[:-1]).all())
        rt = (R.unwarp(z64, near, far) - s64).abs()
        assert float(rt[1:-1].max()) <= 1e-9
        # the end points: W(0) = 1/gn and W(1) = 1/gf are near and far only to the rounding of gn, gf, and W^-1 clamps to [near, far]
        assert float(rt.max()) <= 2 * EPS / (1.0 - near / far)
        s32 = torch.linspace(0.0, 1.0, 4097)                                                              # steps far above the rounding
        z32 = R.warp(s32, near, far)
        assert bool((z32[1:] > z32[:-1]).all())
        # fp32 round trip: the inverse's own bound + the forward error carried through dW^-1/dz = 1 / (z^2 (gn - gf)) <= 1 / (z near (gn - gf))
        back = R.unwarp(z32, near, far)
        assert float((back.double() - s32.double()).abs().max()) <= 16 * EPS / (1.0 - near / far)
        assert float(back.min()) >= 0.0 and float(back.max()) <= 1.0 + 2 * EPS / (1.0 - near / far)


def test_fp32_step_by_step_warp_stays_within_the_derived_bounds_of_fp64():
    """The bounds the GPU test applies to the kernel (five roundings of positive terms, 8 ulp/2 with room for the division; the inverse's
    cancellation factor 1 / (1 - near/far)), here on the numpy emulation: 2e6 random s plus the end points per (near, far)."""
    rng = np.random.default_rng(5)
    for near, far in PAIRS:
        s = np.concatenate((rng.random(2_000_000, dtype=np.float32), np.array([0.0, 1.0, 1.0 - EPS, EPS], dtype=np.float32)))
        z32 = R.warp_np32(s, near, far)
        z64 = R.warp(torch.from_numpy(s).double(), near, far).numpy()
        fwd = float(np.max(np.abs(z32.astype(np.float64) - z64) / z64))
        assert fwd <= 8 * EPS, (near, far, fwd / EPS)
        assert np.array_equal(z32, R.warp(torch.from_numpy(s), near, far).numpy())                        # torch fp32 == the numpy steps
        zin = z32                                                                                         # fp32 depths inside [near, far]
        s32 = R.unwarp_np32(zin, near, far)
        s64 = R.unwarp(torch.from_numpy(zin).double(), near, far).numpy()
        inv = float(np.max(np.abs(s32.astype(np.float64) - s64)))
        assert inv <= 8 * EPS / (1.0 - near / far), (near, far, inv / EPS)
        assert np.array_equal(s32, R.unwarp(torch.from_numpy(zin), near, far).numpy())
        print("warp fp32 vs fp64 (%g, %g): forward %.2f x 2^-24 relative, inverse %.2f x 2^-24 absolute" % (near, far, fwd / EPS, inv / EPS))


def test_coarse_s_never_exceeds_one():
    """At the sizes the project uses (render: 64; the tests: 32, 64, 130; every power of two) the largest s_j -- u = 1 - 2^-24, j = C - 1 -- is
    at most 1, and exactly 1.0 at C = 64: hence the clamp in W.  For other C, r = fp32(1/C) may be rounded UP and the top s_j lands one ulp
    above 1 (C = 56 does): the same clamp absorbs it, W(s_j) = W(1)."""
    for C in (4, 8, 16, 32, 64, 128, 256, 130):
        assert float(R.coarse_s(torch.full((1, C), 1.0 - EPS)).max()) <= 1.0, C
    assert float(R.coarse_s(torch.full((1, 64), 1.0 - EPS))[0, -1]) == 1.0
    over = []
    for C in range(3, 257):
        top = R.coarse_s(torch.full((1, C), 1.0 - EPS))
        assert float(top.max()) <= 1.0 + 2.0 ** -23, C                                                    # never more than one ulp of 1
        if float(top.max()) > 1.0:
            over.append(C)
        assert torch.equal(R.warp(top[:, -1:], 0.2, 1000.0), R.warp(torch.ones(1, 1), 0.2, 1000.0)) or float(top.max()) < 1.0
        low = R.coarse_s(torch.zeros((1, C)))
        assert float(low[0, 0]) == 0.0 and bool((low[0, 1:] > low[0, :-1]).all())
    assert 56 in over


def test_spacing_is_keyword_only_and_linear_by_default():
    from nerf_amd import parallel, procedures, training, utils
    for fn in (procedures.render_image, procedures._render_rays_by_calls, parallel.render_image_sharded, training.TrainStep.__init__):
        prm = inspect.signature(fn).parameters["spacing"]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == "linear", fn
    s = torch.linspace(0.0, 1.0, 9)[None]
    assert torch.equal(utils.warp_depths(s, 2.0, 6.0, "linear"), 2.0 + s * 4.0)                          # plain torch: no device needed
    assert torch.allclose(utils.unwarp_depths(utils.warp_depths(s, 2.0, 6.0, "linear"), 2.0, 6.0, "linear"), s, atol=1e-6)
    with pytest.raises(ValueError):
        procedures._check_spacing("log", 2.0, 6.0)
    with pytest.raises(ValueError):
        procedures._check_spacing("disparity", 0.0, 6.0)
    assert procedures._check_spacing("linear", 0.0, 0.0) is False and procedures._check_spacing("disparity", 0.2, 1e6) is True
