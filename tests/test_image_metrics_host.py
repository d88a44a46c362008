"""Image metrics without a GPU: the fp64 specification (tests/image_metrics_ref.py) against an independent 121-tap restatement and hand
cases; the fp32 emulation of the shipped algorithm inside the derived bounds at every shape of the device sweep; eight planted faults,
each caught there by the check the device test uses; the host side of the interface.

Measured here (worst err / tol over the sweep's shapes and both input kinds; `pytest -s` prints every figure):
    emulation against the bounds      map 0.056, ssim 0.019, mse 0.037     (the bounds are worst-case sums of 27 roundings per term;
                                                                            roundings add like a random walk, hence the margin)
    planted faults                    the factors stand in the docstring of test_planted_faults_are_caught_at_the_device_shapes"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import image_metrics_ref as R
from conftest import gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    from nerf_amd import _lib
    return _lib.IMAGE_METRICS_TILE + (_lib.IMAGE_METRICS_SEGMENT_H,)


def _sweep():
    return [(s, k) for s in R.sweep_shapes(*_tile()) for k in R.INPUT_KINDS]


_SPEC_CACHE = {}


def _case(shape, kind):
    """inputs, specification and bounds of one sweep case, computed once"""
    key = (tuple(shape), kind)
    if key not in _SPEC_CACHE:
        pred, target = R.make_inputs(shape, kind)
        sp = R.spec(pred, target)
        _SPEC_CACHE[key] = (pred, target, sp, R.bounds(sp))
    return _SPEC_CACHE[key]


# ------------------------------------------------------------------------------------------------ the specification
def test_spec_equals_full_2d_window():
    """separable fp64 spec == the 121-tap window through scipy.signal.convolve2d(mode="valid"), to fp64 rounding"""
    from scipy.signal import convolve2d
    g = R.window64()
    k2 = np.outer(g, g)[::-1, ::-1]                                                          # convolve2d flips; the window is symmetric anyway
    for shape, kind in (((2, 3, 13, 75), "textured"), ((1, 1, 27, 75), "wide"), ((1, 3, 11, 11), "textured")):
        pred, target = R.make_inputs(shape, kind)
        sp = R.spec(pred, target)
        x, y = pred.astype(np.float64), target.astype(np.float64)
        for v in range(shape[0]):
            for c in range(shape[1]):
                cv = lambda a: convolve2d(a, k2, mode="valid")
                mx, my = cv(x[v, c]), cv(y[v, c])
                vx, vy, cxy = cv(x[v, c] ** 2) - mx ** 2, cv(y[v, c] ** 2) - my ** 2, cv(x[v, c] * y[v, c]) - mx * my
                want = (2 * mx * my + R.C1) * (2 * cxy + R.C2) / ((mx ** 2 + my ** 2 + R.C1) * (vx + vy + R.C2))
                assert want.shape == (shape[2] - 10, shape[3] - 10)
                # cancellation in the variances at fp64: 121 terms of <= 2.25, 2^-53 each, over a denominator >= C2
                assert np.max(np.abs(sp["ssim_map"][v, c] - want)) <= 1e-11
        assert np.allclose(sp["mse"], ((x - y) ** 2).reshape(shape[0], -1).mean(1), rtol=1e-15, atol=0)


def test_hand_cases():
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 1, (2, 3, 14, 17)).astype(np.float32)
    sp = R.spec(x, x)                                                                        # identical images
    assert np.max(np.abs(sp["ssim_map"] - 1.0)) <= 1e-12 and (sp["mse"] == 0).all() and np.isposinf(sp["psnr"]).all()
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.9, 0.9), (1.5, -0.5)):                          # two constant images
        sp = R.spec(np.full((1, 2, 12, 13), a, np.float32), np.full((1, 2, 12, 13), b, np.float32))
        assert np.max(np.abs(sp["ssim_map"] - R.constant_ssim(a, b))) <= 1e-12
        assert abs(sp["mse"][0] - (a - b) ** 2) <= 1e-15 and abs(sp["ssim"][0] - R.constant_ssim(a, b)) <= 1e-12
    sp = R.spec(*R.make_inputs((1, 1, 11, 11), "textured"))                                  # 11 x 11: exactly one position
    assert sp["ssim_map"].shape == (1, 1, 1, 1) and sp["ssim"][0] == sp["ssim_map"][0, 0, 0, 0]
    assert R.spec(x[0], x[0])["ssim_map"].shape == (1, 3, 4, 7)                               # (C, H, W) is one view
    g = R.window32()
    assert g.dtype == np.float32 and g.shape == (11,) and (g == g[::-1]).all() and g.argmax() == 5
    assert abs(float(g.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23                          # sums to 1 within an ulp
    assert abs(R.window64().sum() - 1.0) <= 2.0 ** -52
    assert np.allclose(g[5] / g[4], np.exp(1.0 / 4.5), rtol=1e-6)


def test_library_window_is_the_specs():
    """the 11 fp32 constants the launcher hands to the kernel are computed by the same recipe (same bits)"""
    src = open(os.path.join(ROOT, "nerf_amd", "csrc", "image_metrics_kernels.hip")).read()
    assert "exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5))" in src and "(float)(w[i] / sum)" in src
    i = np.arange(11)
    w = np.exp(-((i - 5) * (i - 5)).astype(np.float64) / (2.0 * 1.5 * 1.5))
    assert ((w / w.sum()).astype(np.float32) == R.window32()).all()


# ------------------------------------------------------------------------------------------------ the emulation and the bounds
def test_emulation_inside_bounds_at_every_sweep_shape():
    worst = {"map": 0.0, "ssim": 0.0, "mse": 0.0}
    for shape, kind in _sweep():
        pred, target, sp, tols = _case(shape, kind)
        assert np.isfinite(tols[0]).all(), (shape, kind)                                     # no position of the sweep has an infinite bound
        r = R.ratios(R.emulate(pred, target), sp, tols)
        for k in worst:
            worst[k] = max(worst[k], r[k])
    for k, v in worst.items():
        gate("image_metrics emulation %s: worst err / tol over the sweep" % k, v, 1.0)
    # the bound is not slack by orders of magnitude either: the emulation uses a fair share of it on textured inputs
    assert worst["map"] >= 0.01


def test_bound_is_per_position_loose_on_bright_flat_tight_on_texture():
    """a flat 0.9 image with 1e-4 noise: fp32 errors of ~1e-4 per position are real there (the cancellation against C2), and the bound admits
    them; on textured patches it stays below 2e-5.  One constant could not do both."""
    rng = np.random.default_rng(11)
    flat_t = (0.9 + rng.normal(0, 1e-4, (1, 1, 32, 32))).astype(np.float32)
    flat_p = (0.9 + rng.normal(0, 1e-4, (1, 1, 32, 32))).astype(np.float32)
    sp = R.spec(flat_p, flat_t)
    tols = R.bounds(sp)
    r = R.ratios(R.emulate(flat_p, flat_t), sp, tols)
    gate("image_metrics emulation, flat 0.9 + 1e-4 noise: map err / tol", r["map"], 1.0)
    print("flat image: per-position bound %.2e .. %.2e" % (tols[0].min(), tols[0].max()))
    assert tols[0].min() >= 1e-4
    for shape in R.sweep_shapes(*_tile()):
        assert _case(shape, "textured")[3][0].max() <= 2e-5, shape


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_faults_are_caught_at_the_device_shapes(fault):
    """Each fault, planted into the emulation, fails the device test's own check (R.ratios against the same bounds, the same inputs) at
    EVERY case of the sweep at which it is a fault at all -- one channel cannot tell when channels are averaged, one view not whose target
    is read -- and which has more than one position.  The 11 x 11 case has ONE position per channel: whether a fault moves that one value
    by more than its bound is chance (measured: 6 of 8 do, x1.01 and C2 on the "wide" inputs reach 0.2 and 0.93 of it), so it is printed, not
    asserted.  Smallest factor by which each fault exceeds the bound over the asserted cases, as measured ('*': the map's shape differs
    too, the figure is the mean's):  pad_same 2.1*  window_x1.01 2.1  sigma_1.0 170  taps_7 4.6*  c2_from_0.01 2.3  channel_mean_first 34*
    mean_over_hw 2.3e4  target_of_view_0 1.5e8."""
    smallest, caught = float("inf"), 0
    for shape, kind in _sweep():
        if (fault == "channel_mean_first" and shape[1] == 1) or (fault == "target_of_view_0" and shape[0] == 1):
            continue                                                                         # the identity at this shape, not a fault
        pred, target, sp, tols = _case(shape, kind)
        r = R.ratios(R.emulate(pred, target, fault), sp, tols)
        finite = max(v for v in r.values() if np.isfinite(v))
        print("FAULT %-20s %-18s %-8s exceeds the bound by a factor %9.3g (map %9.3g  ssim %9.3g  mse %9.3g)"
              % (fault, shape, kind, finite, r["map"], r["ssim"], r["mse"]))
        if (shape[2] - 10) * (shape[3] - 10) > 1:
            assert finite > 1.0, (fault, shape, kind, r)                                     # (a changed map shape is caught on top of this)
            smallest = min(smallest, finite)
            caught += 1
    print("FAULT %-20s smallest factor over the %d asserted cases %.3g" % (fault, caught, smallest))
    assert caught >= 4 and smallest > 1.0


# ------------------------------------------------------------------------------------------------ the host side of the interface
def test_abi_rows_and_frozen_layouts():
    from nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    for name, nargs in (("nerf_amd_image_metrics_workspace_bytes", 4), ("nerf_amd_image_metrics", 11)):
        assert header.count(name + "(") >= 1 and name in _lib.SIGNATURES and name in _lib.ADDED_AFTER_125, name
        assert len(_lib.SIGNATURES[name][1]) == nargs and hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
    res, args = _lib.SIGNATURES["nerf_amd_image_metrics"]
    assert res is ctypes.c_int and args[2] is ctypes.c_int64 and args[3:6] == [ctypes.c_int] * 3 and all(a is ctypes.c_void_p for a in args[:2] + args[6:])
    assert _lib.SIGNATURES["nerf_amd_image_metrics_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int])
    assert _lib.lib.nerf_amd_version() == 125 and _lib.EXPECTED_VERSION == 125
    assert ctypes.sizeof(_lib.Samples) == 168 and ctypes.sizeof(_lib.RenderRequest) == 224
    th = int(re.search(r"#define NERF_AMD_IMAGE_METRICS_TILE_H (\d+)", header).group(1))
    tw = int(re.search(r"#define NERF_AMD_IMAGE_METRICS_TILE_W (\d+)", header).group(1))
    sh = int(re.search(r"#define NERF_AMD_IMAGE_METRICS_SEGMENT_H (\d+)", header).group(1))
    assert (th, tw) == tuple(_lib.IMAGE_METRICS_TILE) and sh == _lib.IMAGE_METRICS_SEGMENT_H and sh % th == 0


def test_c_abi_rejects_bad_arguments_without_a_device():
    """NERF_AMD_EINVAL with a message for H or W < 11, non-positive sizes and NULL required pointers: all decided on the host"""
    from nerf_amd import _lib
    lib = _lib.lib
    (th, tw), sh = _lib.IMAGE_METRICS_TILE, _lib.IMAGE_METRICS_SEGMENT_H
    ws = lib.nerf_amd_image_metrics_workspace_bytes                                            # 16 bytes per workgroup = per (plane, segment of rows, strip of columns)
    assert ws(1, 1, 11, 11) == 16 and ws(2, 3, th + 11, tw + 11) == 2 * 3 * 2 * 16 and ws(1, 3, sh + 10, 2 * tw + 10) == 3 * 2 * 16
    assert ws(1, 1, sh + 11, tw + 10) == 2 * 16 and ws(200, 3, 800, 800) == 200 * 3 * (-(-790 // sh)) * (-(-790 // tw)) * 16
    for bad in ((1, 1, 10, 11), (1, 1, 11, 10), (0, 1, 11, 11), (1, 0, 11, 11), (-1, 3, 20, 20), (1, 3, -5, 20), (2 ** 40, 3, 11, 11)):
        assert ws(*bad) == 0, bad
    p = ctypes.c_void_p(4096)                                                                # never dereferenced: every call below is refused first
    call = lib.nerf_amd_image_metrics
    for bad, word in (((1, 1, 10, 11), "at least 11"), ((1, 1, 11, 10), "at least 11"), ((0, 1, 11, 11), "positive"), ((1, 0, 11, 11), "positive"),
                      ((1, 1, 11, 0), "positive"), ((2 ** 40, 3, 11, 11), "too many segments")):
        rc = call(p, p, *bad, p, p, None, p, None)
        assert rc != 0 and word in lib.nerf_amd_last_error().decode(), (bad, rc, lib.nerf_amd_last_error())
    for k in (0, 1, 6, 7, 9):                                                                # pred, target, mse_out, ssim_out, workspace
        a = [p, p, 1, 1, 11, 11, p, p, None, p, None]
        a[k] = None
        assert call(*a) != 0 and "NULL" in lib.nerf_amd_last_error().decode(), k


class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) before the arguments were refused" % name)


def test_every_value_error_is_raised_before_a_launch(monkeypatch):
    from nerf_amd import metrics, ops
    monkeypatch.setattr(ops, "lib", _NoLaunch())
    ok = torch.zeros(1, 3, 12, 12)
    for pred, target, word in ((ok.double(), ok, "float32"), (ok, ok.half(), "float32"), (ok[0, 0], ok[0, 0], r"\(V, C, H, W\)"),
                               (ok.reshape(1, 1, 3, 12, 12), ok.reshape(1, 1, 3, 12, 12), r"\(V, C, H, W\)"),
                               (ok.transpose(2, 3), ok.transpose(2, 3), "contiguous"), (ok[:, :, :, ::2].expand(1, 3, 12, 6), ok[:, :, :, :6].contiguous(), "contiguous"),
                               (ok, torch.zeros(1, 3, 12, 13), "one shape"), (ok[0], ok, "one shape"),
                               (torch.zeros(1, 3, 10, 12), torch.zeros(1, 3, 10, 12), "at least 11"), (torch.zeros(3, 12, 10), torch.zeros(3, 12, 10), "at least 11"),
                               (torch.zeros(0, 3, 12, 12), torch.zeros(0, 3, 12, 12), "at least one view"), (np.zeros((1, 3, 12, 12), np.float32), ok, "torch.Tensor"),
                               (ok, ok, "HIP device")):
        for fn in (ops.image_metrics, metrics.image_metrics, metrics.SSIM(), metrics.PSNR()):
            with pytest.raises(ValueError, match=word):
                fn(pred, target)
    with pytest.raises(ValueError, match="HIP device"):
        ops.image_metrics(ok, ok, want_map=True)
    with pytest.raises(ValueError, match=r"\(V, 3, H, W\)|HIP device"):
        metrics.evaluate_views(None, None, torch.zeros(2, 1, 12, 12), torch.zeros(2, 3, 4), 10.0, 2.0, 6.0)
    with pytest.raises(ValueError, match="not a keyword"):
        metrics.evaluate_views(None, None, ok, torch.zeros(1, 3, 4), 10.0, 2.0, 6.0, image_size=(12, 12))


def test_metrics_are_forward_only(monkeypatch):
    """a backward is out of scope: inputs that require grad raise instead of returning a tensor without a graph"""
    from nerf_amd import metrics, ops
    monkeypatch.setattr(ops, "lib", _NoLaunch())
    x = torch.zeros(1, 3, 12, 12, requires_grad=True)
    for fn in (metrics.image_metrics, metrics.SSIM(), metrics.PSNR()):
        with pytest.raises(RuntimeError, match="forward only"):
            fn(x, torch.zeros(1, 3, 12, 12))
        with torch.no_grad(), pytest.raises(ValueError, match="HIP device"):                # under no_grad the call goes on (and stops at the device check here)
            fn(x, torch.zeros(1, 3, 12, 12))
    assert "ln 10" in metrics.__doc__ and "LossPSNR" in metrics.__doc__


def test_eval_ssim_flag_parses_and_defaults_to_off():
    import inspect
    from nerf_amd import metrics, procedures
    p = procedures.get_parser()
    assert p.parse_args([]).eval_ssim is False and p.parse_args(["--eval_ssim"]).eval_ssim is True
    assert p.parse_args(["-e", "--eval_ssim", "--skip_empty", "0.01"]).skip_empty == 0.01
    sig = inspect.signature(metrics.evaluate_views).parameters
    assert [k for k, v in sig.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == ["network", "prop_net", "images", "poses", "focal", "near", "far"]
    assert sig["sample_num"].default == 128 and sig["white_bkg"].default is False and sig["seed"].default is None and sig["camera"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("sample_num", "white_bkg", "seed", "camera"))
    assert "metrics" not in " ".join(os.listdir(os.path.join(ROOT, "compat", "nerf")))
