"""Interlevel loss (Mip-NeRF 360 L_prop), host side (no GPU): the fp64 specification of tests/interlevel_ref.py equals the brute-force
overlap mask, its inputs are not vacuous, InterlevelLoss on CPU tensors evaluates the specification, the C-ABI carries the two entry
points (validated before any HIP call, ABI number unchanged), and TrainStep / render_image take and validate the new keywords."""
import inspect
import os
import subprocess
import sys

import pytest
import torch

import interlevel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = 17
VARIANTS = [(o, t) for o in (False, True) for t in (False, True)]


@pytest.fixture(scope="module")
def evaluated():
    """(M, K, open, ties) -> (inputs, spec (bounds, loss, grad)) once for the module"""
    out = {}
    for M, K in R.HOST_SHAPES:
        for open_form, ties in VARIANTS:
            x = R.make_inputs(RAYS, M, K, open_form, ties, 100 * M + K)
            out[(M, K, open_form, ties)] = (x, R.evaluate(*x))
    return out


@pytest.mark.parametrize("M,K", R.HOST_SHAPES)
def test_spec_equals_the_brute_force_overlap_mask(evaluated, M, K):
    """prefix sum + searchsorted against the (N, M, K) mask in fp64: bounds, loss and gradient within 1e-12 absolute"""
    for open_form, ties in VARIANTS:
        x, (b, l, g) = evaluated[(M, K, open_form, ties)]
        bb, lb, gb = R.evaluate(*x, bounds_fn=R.brute_bounds)
        err = ((b - bb).abs().max().item(), abs(l - lb), (g - gb).abs().max().item())
        print("interlevel spec vs brute force (M %d, K %d, open %d, ties %d): bounds %.3g loss %.3g grad %.3g" % (M, K, open_form, ties, *err))
        assert max(err) <= 1e-12, (open_form, ties, err)


def test_ties_option_makes_exact_edge_ties():
    w, t, w_prop, t_prop = R.make_inputs(RAYS, 63, 65, False, True, 5)
    assert (t[:, :, None] == t_prop[:, None, :]).any(-1).sum(-1).min().item() >= 30
    assert bool((t[:, 1:] >= t[:, :-1]).all()) and bool((t_prop[:, 1:] >= t_prop[:, :-1]).all())


def test_inputs_are_not_vacuous(evaluated):
    """on the spec's own output: >= 10 % of the fine intervals active (w_i > bound_i) where M, K >= 2, >= 20 % of the gradient entries
    non-zero where K >= 32 -- a loss that is identically zero, or a gradient that is, would pass every comparison"""
    for (M, K, open_form, ties), ((w, t, w_prop, t_prop), (b, l, g)) in evaluated.items():
        active = (w.double() > b).double().mean().item()
        nonzero = (g != 0).double().mean().item()
        print("interlevel inputs (M %d, K %d, open %d, ties %d): active %.3f, non-zero gradient %.3f" % (M, K, open_form, ties, active, nonzero))
        if M >= 2 and K >= 2:
            assert active >= 0.10, (M, K, open_form, ties, active)
        if K >= 32:
            assert nonzero >= 0.20, (M, K, open_form, ties, nonzero)


def test_definition_on_a_hand_made_ray():
    """one ray written out: touching counts as overlapping, outside the span the bound is 0, the open form's last interval reaches +inf"""
    t = torch.tensor([[0.0, 1.0, 2.0, 3.0, 5.0, 9.0]], dtype=torch.float64)
    e = torch.tensor([[1.0, 2.5, 3.0, 4.0]], dtype=torch.float64)
    p = torch.tensor([[0.5, 0.25, 0.125]], dtype=torch.float64)
    # [0,1] touches [1,2.5); [1,2] lies in it; [2,3] overlaps [1,2.5) and [2.5,3) and touches [3,4); [3,5] starts at lo(3) = 2: [3,4) alone;
    # [5,9] is past the closed span
    assert R.spec_bounds(t, p, e).tolist() == [[0.5, 0.5, 0.875, 0.125, 0.0]]
    assert R.brute_bounds(t, p, e).tolist() == [[0.5, 0.5, 0.875, 0.125, 0.0]]
    # open form: depths 1, 2.5, 3 -- the last weight covers [3, +inf)
    assert R.spec_bounds(t, p, e[:, :3]).tolist() == [[0.5, 0.5, 0.875, 0.125, 0.125]]
    assert R.brute_bounds(t, p, e[:, :3]).tolist() == [[0.5, 0.5, 0.875, 0.125, 0.125]]


@pytest.mark.parametrize("M,K", [(1, 1), (3, 64), (63, 65), (128, 64)])
def test_interlevel_loss_on_cpu_tensors_is_the_spec(evaluated, M, K):
    from nerf_amd.addtional import InterlevelLoss
    for open_form, ties in VARIANTS:
        (w, t, w_prop, t_prop), (b, l, g) = evaluated[(M, K, open_form, ties)]
        p = w_prop.double().requires_grad_(True)
        ww = w.double().requires_grad_(True)
        loss = InterlevelLoss(0.5)(ww, t.double(), p, t_prop.double())
        loss.backward()
        assert ww.grad is None                                                       # the fine weights are constants
        assert abs(loss.item() - 0.5 * l) <= 1e-12 and (p.grad - 0.5 * g).abs().max().item() <= 1e-12
        assert (InterlevelLoss.bounds(t.double(), w_prop.double(), t_prop.double()) - b).abs().max().item() <= 1e-12
        l32 = InterlevelLoss()(w, t, w_prop, t_prop)
        assert l32.dtype == torch.float32 and abs(l32.item() - l) <= 1e-4 * max(l, 1e-3)


def test_shim_serves_the_interlevel_loss():
    compat = os.path.join(ROOT, "compat")
    code = ("import sys, nerf.addtional as shim, nerf_amd.addtional as real\n"
            "from nerf.addtional import InterlevelLoss\n"
            "assert InterlevelLoss is real.InterlevelLoss\n"
            "print('resolved')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, compat]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "resolved" in r.stdout, r.stderr[-2000:]


def test_symbols_are_declared_bound_and_the_abi_number_stays():
    from nerf_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    for name in ("nerf_amd_interlevel_loss", "nerf_amd_interlevel_loss_backward"):
        assert "int %s(" % name in header and name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert "#define NERF_AMD_INTERLEVEL_MAX 1024" in header
    assert "#define NERF_AMD_INTERLEVEL_WORKSPACE_FLOATS %d" % ops.INTERLEVEL_WORKSPACE_FLOATS in header
    assert ops.INTERLEVEL_MAX == 1024
    assert _lib.lib.nerf_amd_version() == 125


def test_interlevel_abi_validates_before_any_hip_call():
    import ctypes as C
    from nerf_amd import _lib
    lib = _lib.lib
    bufs = [(C.c_float * 64)() for _ in range(8)]
    w, t, wp, tp, out, ws, g, d = (C.cast(b, C.c_void_p) for b in bufs)                  # host memory: a call that got past the checks would fail in HIP
    fwd = lambda *a: lib.nerf_amd_interlevel_loss(*a, None)                              # noqa: E731
    bwd = lambda *a: lib.nerf_amd_interlevel_loss_backward(*a, None)                     # noqa: E731
    for n, m, k, kp in ((4, 0, 4, 5), (4, 1025, 4, 5), (4, 4, 0, 1), (4, 4, 1025, 1026), (4, 4, 8, 7), (4, 4, 8, 10), (-1, 4, 8, 9)):
        assert fwd(w, t, wp, tp, n, m, k, kp, 1.0, out, None, ws) == -1, (n, m, k, kp)
        assert lib.nerf_amd_last_error()
        assert bwd(w, t, wp, tp, n, m, k, kp, 1.0, g, d) == -1, (n, m, k, kp)
    assert fwd(w, t, wp, tp, 4, 1025, 4, 5, 1.0, out, None, ws) == -1 and b"1024" in lib.nerf_amd_last_error()
    full = [w, t, wp, tp, 4, 4, 8, 9, 1.0, out, None, ws]
    for hole in (0, 1, 2, 3, 9, 11):                                                      # (bounds_out, slot 10, may be NULL)
        a = list(full)
        a[hole] = None
        assert fwd(*a) == -1 and b"NULL" in lib.nerf_amd_last_error(), hole
    full = [w, t, wp, tp, 4, 4, 8, 8, 1.0, g, d]
    for hole in (0, 1, 2, 3, 9, 10):
        a = list(full)
        a[hole] = None
        assert bwd(*a) == -1 and b"NULL" in lib.nerf_amd_last_error(), hole


def test_ops_refuse_mismatched_shapes_and_cpu_tensors():
    from nerf_amd import ops
    w, t, w_prop, t_prop = R.make_inputs(3, 4, 5, False, False, 0)
    with pytest.raises(RuntimeError):
        ops.interlevel_loss(w, t, w_prop, t_prop, 1.0)                                   # no CPU path in ops (InterlevelLoss has the torch expression)


def test_train_step_and_render_image_take_the_keywords():
    from nerf_amd import procedures
    from nerf_amd.training import TrainStep
    p = inspect.signature(TrainStep.__init__).parameters
    for name, default in (("prop_loss", "reference"), ("prop_rounds", 1), ("prop_pnum", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    for fn in (procedures.render_image, procedures._render_rays_by_calls):
        q = inspect.signature(fn).parameters
        assert q["prop_rounds"].kind is inspect.Parameter.KEYWORD_ONLY and q["prop_rounds"].default == 1
        assert q["prop_pnum"].kind is inspect.Parameter.KEYWORD_ONLY and q["prop_pnum"].default is None
        assert list(q).index("prop_rounds") > list(q).index("spacing")


def test_render_image_validates_the_rounds_before_touching_a_device():
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.procedures import render_image
    from nerf_amd.ref_model import RefNeRF
    prop, mip, pose = ProposalNetwork(10, 256), MipNeRF(10, 4, 256), torch.eye(4)[:3]
    for rng in ("reference", "device"):
        with pytest.raises(ValueError, match="philox"):
            render_image(mip, prop, pose, 40, 50.0, 2.0, 6.0, 64, rng=rng, prop_rounds=2)
    with pytest.raises(ValueError, match="prop_rounds"):
        render_image(mip, prop, pose, 40, 50.0, 2.0, 6.0, 64, prop_rounds=3)
    with pytest.raises(ValueError, match="prop_pnum"):
        render_image(mip, prop, pose, 40, 50.0, 2.0, 6.0, 64, prop_rounds=2, prop_pnum=0)
    with pytest.raises(NotImplementedError):
        render_image(RefNeRF(10, 4), prop, pose, 40, 50.0, 2.0, 6.0, 64, prop_rounds=2)
