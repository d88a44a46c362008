"""The regulariser kernels of nerf_amd/csrc/sample_kernels.hip -- distortion_loss_kernel<0|1>, distortion_loss_backward_kernel<0|1>,
interlevel_loss_kernel, interlevel_loss_backward_kernel -- against the fp64 specification and the per-element bounds of
tests/regularizer_ref.py (derived there; tests/test_regularizer_ref_host.py runs the SAME check functions over the torch emulation on
the CPU).  Every element of every output of a case goes through ONE gate(name, max(err / tol), 1.0) whose name carries kernel, mode,
family, shape, g, scale and each output's own figure; the exact statements -- zero bounds (equality), the NaN pattern, guard elements,
unrequested outputs, inputs bit-unchanged, two runs bit-equal -- are counted and go through one gate(name, count, 0) per test, which
names the violated ones.  Next to each case an `EMUL` line gives the emulation's figures for the same inputs and bounds, on the device.

THE SHAPES AND THE PATHS THEY REACH
  distortion row lengths S (M = S - 1 intervals), both modes, every family the mode admits:
    2, 3, 4        one interval (mode 0: r = 0, NaN by contract); two intervals (P constant in t: the four terms of the mode-0 depth
                   gradient cancel exactly); three intervals
    64, 65, 66     the lane boundary: M = 63 fills lanes 0..62, M = 64 the whole first register, M = 65 starts register 1, whose lane 0
                   takes its lower part through dist_from_below's hand-over from lane 63 of register 0
    128, 129, 130  the register-block boundary: M = 127; M = 128 = 64 DIST_R, where column M falls past the last register block and is
                   written from carry_w / carry_t (the `M % 128 == 0` branch); M = 129 starts a second block
    257            M = 256: the second block ends exactly (column M from the carry again)
    683, 684       the mode-0 backward's dynamic LDS, 4 waves x 24 bytes x M: 65 472 bytes at M = 682, 65 568 at M = 683 -- the two sides
                   of the 64 KiB switch (allow_dynamic_lds)
    1024           the limit, 96 KiB
  distortion N: 1, 3, 4, 5 (workgroups of four waves: part of one, exactly one, one and a wave); 4097 at S = 65 (1025 workgroups: past
    the forward's cap of 1024, DIST_BLOCKS); 8197 at S = 65 (2050 workgroups: past blocks_for's cap of 2048, so rays 8192.. are the
    second grid-stride trip of their wave -- the LDS row re-staged, carry_w / carry_t reset, pass 1 over u, q repeated); 8197 at
    S = 129 in mode 0 as well, the one row length at which a carry that is NOT reset would show (M % 128 == 0)
  interlevel (M, K): interlevel_ref.GPU_SHAPES; (1023, 1023) | (1024, 1024): 16 384 | 16 400 bytes per wave, four-wave | two-wave forward
    (il_waves); (682, 681) | (682, 682): 12 (M + K) + 24 = 16 380 | 16 392 bytes, four-wave | two-wave backward
  interlevel N: 1, 5; 4097 (past the forward's cap of 1024 workgroups, IL_BLOCKS); 8197 at (63, 65) (past blocks_for's cap with four
    waves); 4099 at (682, 682) (past it with two waves: 2050 workgroups)
  g in {1, 0.37, -2.5} as a 0-dim device tensor and scale in {1, 0.25, 3} cycle through the cases (regularizer_ref.pick)."""
import ctypes as C

import pytest
import torch

import interlevel_ref as R
import regularizer_ref as G
from conftest import gate

pytestmark = pytest.mark.gpu
DIST_S = (2, 3, 4, 64, 65, 66, 128, 129, 130, 257, 683, 684, 1024)
IL_SHAPES = R.GPU_SHAPES + ((1023, 1023), (682, 681), (682, 682))
GUARD = 256
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


class Ops:
    """the kernels through nerf_amd.ops, with the interface of regularizer_ref.Emulation"""

    def distortion_loss(self, w, t, mode, scale):
        from nerf_amd import ops
        return ops.distortion_loss(w, t, mode, scale)

    def distortion_backward(self, g, w, t, mode, scale, need=(True, True)):
        from nerf_amd import ops
        return ops.distortion_loss_backward(g, w, t, mode, scale, need)

    def interlevel_loss(self, w, t, w_prop, t_prop, scale):
        from nerf_amd import ops
        return ops.interlevel_loss(w, t, w_prop, t_prop, scale, want_bounds=True)

    def interlevel_backward(self, g, w, t, w_prop, t_prop, scale):
        from nerf_amd import ops
        return ops.interlevel_loss_backward(g, w, t, w_prop, t_prop, scale)


OPS, EMU = Ops(), G.Emulation(cap=2048)


_EXACT = []


def _exact(name, count):
    """an exact statement (limit 0): recorded here, gated once per test by _exact_gate, named there if violated"""
    _EXACT.append((name, float(count)))


@pytest.fixture(autouse=True)
def _exact_gate(request):
    del _EXACT[:]
    yield
    if not _EXACT:
        return
    bad = [n for n, c in _EXACT if c != 0]
    gate("%s: %d exact statements, violated (elements)%s" % (request.node.name, len(_EXACT), ": " + "; ".join(bad) if bad else ""),
         sum(c for _, c in _EXACT), 0.0)


def _figures(items):
    return " ".join("%s %.3f" % (n.split()[-1], v) for n, v, l in items if l)


def _check(kind, tag, x, run, ref, parts=None):
    """one case -> ONE gate line: the worst err / tol over the outputs, each output's own figure in the gate's name, and an `EMUL` line
    with the emulation's figures for the same inputs and bounds.  The exact statements of the case -- zero bounds and the NaN pattern
    (which worst() also turns into inf), inputs unchanged, two runs bit-equal -- are counted into the test's exact gate"""
    before = [v.clone() for v in x]
    got, again = run(OPS), run(OPS)
    torch.cuda.synchronize()
    _exact(tag + " inputs changed", sum(int((a != b).sum()) for a, b in zip(before, x)))
    _exact(tag + " two runs differ", sum(int((~((got[k] == again[k]) | (torch.isnan(got[k]) & torch.isnan(again[k])))).sum()) for k in got))
    items, emu = G.compare(tag, got, ref), G.compare(tag, run(EMU), ref)
    for name, sl in (parts or {}).items():                                           # a named part of the batch, compared like the whole
        items += [("%s %s:%s" % (tag, name, k), G.worst(got[k][sl], ref[k][0][sl], ref[k][1][sl]), 1.0) for k in got if got[k].dim() == 2]
    for (name, value, limit), (_, evalue, _) in zip(items, emu):
        if limit:
            key = kind + " " + name.split()[-1]
            WORST[key] = (max(WORST.get(key, (0.0, 0.0))[0], value), max(WORST.get(key, (0.0, 0.0))[1], evalue))
        else:
            _exact(name, value)
    print("EMUL %s emulation [%s]" % (tag, _figures(emu)))
    gate("%s [%s]" % (tag, _figures(items)), max(v for _, v, l in items if l), 1.0)
    return got


def _dist(family, N, S, mode, parts=None):
    tag, (w, t), g, scale = G.dist_case(family, N, S, mode)
    w, t = w.cuda(), t.cuda()
    ref = G.dist_ref(w, t, mode, g, scale)
    got = _check("distortion mode %d" % mode, tag, (w, t), lambda impl: G.run_dist(impl, w, t, mode, g, scale), ref, parts)
    return (w, t), g, scale, ref, got


def _il(family, N, M, K, open_form, parts=None):
    tag, x, g, scale = G.il_case(family, N, M, K, open_form)
    x = tuple(v.cuda() for v in x)
    ref = G.il_ref(*x, g, scale)
    got = _check("interlevel", tag, x, lambda impl: G.run_il(impl, x, g, scale), ref, parts)
    return x, g, scale, ref, got


# ------------------------------------------------------------------------------------------------ distortion
@pytest.mark.parametrize("S", DIST_S)
@pytest.mark.parametrize("mode", [0, 1])
def test_distortion_row_lengths(mode, S):
    """every row length of the table in the module docstring, every family the mode admits, five rays (nine in `degenerate`); the
    `degenerate` family is compared whole: in mode 0 ray 2's rows and the loss are NaN and every other ray is inside its bounds"""
    for family in G.DIST_FAMILIES[mode]:
        (w, t), g, scale, ref, got = _dist(family, 5, S, mode)
        if family == "degenerate" and mode == 0 and S > 2:
            for k in ("d_w", "d_t"):
                nan = torch.isnan(got[k])
                _exact("distortion mode=0 degenerate S=%d %s NaN outside ray 2 / finite inside" % (S, k),
                       int(nan[:2].sum()) + int(nan[3:].sum()) + int((~nan[2]).sum()))
            assert bool(torch.isnan(got["loss"]))


@pytest.mark.parametrize("N", [1, 3, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_distortion_partly_filled_workgroups(mode, N):
    """N = 1, 3, 4: one wave, three waves, exactly the four waves of a workgroup (5 rays is the sweep above)"""
    for S in (65, 130):
        for family in ("uniform", "clustered"):
            _dist(family, N, S, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_distortion_past_the_forward_grid_cap(mode):
    """4097 rays at S = 65: 1025 workgroups of rays against the forward's 1024 (DIST_BLOCKS): workgroup 0 sums a second trip"""
    for family in ("uniform", "peaked"):
        _dist(family, 4097, 65, mode)


@pytest.mark.parametrize("mode,S", [(0, 65), (1, 65), (0, 129)])
def test_distortion_past_the_backward_grid_cap(mode, S):
    """8197 rays: 2050 workgroups of rays against blocks_for's 2048, so rays 8192..8196 are second trips of the waves of workgroups 0 and
    1 -- the LDS row re-staged, carry_w / carry_t reset, (mode 0) pass 1 repeated.  Those rays are gated on their own as well.  S = 129
    (M = 128) is where a carry that was not reset would reach column 0 of the second-trip ray"""
    for family in (("uniform", "clustered") if S == 65 else ("uniform",)):
        _dist(family, 8197, S, mode, parts={"second-trip rays 8192..": slice(8192, None), "first-trip rays of the same waves": slice(0, 8)})


# ------------------------------------------------------------------------------------------------ interlevel
@pytest.mark.parametrize("M,K", IL_SHAPES)
def test_interlevel_shapes(M, K):
    """every (M, K) of the table, closed and open form, every family, five rays (nine in `degenerate`); N = 1 on two families"""
    for open_form in (False, True):
        for family in G.IL_FAMILIES:
            _il(family, 5, M, K, open_form)
        for family in ("uniform", "ties"):
            _il(family, 1, M, K, open_form)


@pytest.mark.parametrize("N,M,K", [(4097, 63, 65), (4097, 128, 64), (8197, 63, 65), (4099, 682, 682)])
def test_interlevel_past_the_grid_caps(N, M, K):
    """4097: 1025 four-wave workgroups against the forward's 1024 (IL_BLOCKS); 8197 at (63, 65): 2050 four-wave workgroups against the
    backward's 2048 (blocks_for); 4099 at (682, 682): 2050 TWO-wave workgroups of the backward against the same cap.  The rays of the
    second trip are gated on their own as well"""
    first = 8192 if N == 8197 else 4096
    for open_form in (False, True):
        for family in ("uniform", "ties"):
            _il(family, N, M, K, open_form, parts={"second-trip rays %d.." % first: slice(first, None)})


def test_interlevel_bounds_outside_a_closed_span_and_empty_ranges_are_exact():
    """fine rows wholly below and wholly above a closed proposal span: every bound is the exact 0 (hi == lo), every d_w_prop entry the
    stored constant 0 (i1 <= i0 never holds a fine interval); the bounds say so (tol = 0) and the kernels agree"""
    tag, x, g, scale = G.il_case("clustered", 6, 65, 63, False)
    w, t, w_prop, t_prop = (v.cuda() for v in x)
    t = torch.cat((t[:3] - 10.0, t[3:] + 10.0)).contiguous()
    ref = G.il_ref(w, t, w_prop, t_prop, g, scale)
    assert bool((ref["bounds"][1] == 0).all()) and bool((ref["d_w_prop"][1] == 0).all())
    got = _check("interlevel", tag + " outside the span", (w, t, w_prop, t_prop), lambda impl: G.run_il(impl, (w, t, w_prop, t_prop), g, scale), ref)
    assert bool((got["bounds"] == 0).all()) and bool((got["d_w_prop"] == 0).all())


# ------------------------------------------------------------------------------------------------ the C ABI: guards, unrequested outputs
def _ptr(x):
    return C.c_void_p(x.data_ptr())


def _arena(n):
    return torch.full((n + 2 * GUARD,), G.POISON, device="cuda")


def _guards_intact(a):
    return int((a[:GUARD] != G.POISON).sum()) + int((a[-GUARD:] != G.POISON).sum())


@pytest.mark.parametrize("mode,N,S", [(0, 5, 129), (0, 5, 130), (1, 5, 129), (1, 5, 65), (0, 8197, 65), (1, 8197, 65)])
def test_distortion_abi_guards_and_unrequested_gradients(mode, N, S):
    """nerf_amd_distortion_loss[_backward] called directly on buffers with poisoned guard elements on both sides: nothing around an output
    is written (column M from the carry at S = 129, the second trip at N = 8197), a gradient that is not requested (NULL) leaves its
    would-be buffer poisoned, and what is written equals the ops' result bit for bit"""
    from nerf_amd import ops
    from nerf_amd._lib import lib
    tag, (w, t), g, scale = G.dist_case("clustered", N, S, mode)
    w, t = w.cuda(), t.cuda()
    gt = torch.tensor([g], device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ws, out = torch.empty(ops.DISTORTION_WORKSPACE_FLOATS, device="cuda"), _arena(1)
    assert lib.nerf_amd_distortion_loss(_ptr(w), _ptr(t), N, S, mode, scale, _ptr(out[GUARD:]), _ptr(ws), stream) == 0
    want_w, want_t = ops.distortion_loss_backward(gt.reshape(()), w, t, mode, scale)
    torch.cuda.synchronize()
    _exact(tag + " ABI loss guards written", _guards_intact(out))
    assert torch.equal(out[GUARD], ops.distortion_loss(w, t, mode, scale))
    for need_w, need_t in ((True, True), (True, False), (False, True)):
        aw, at = _arena(w.numel()), _arena(t.numel())
        assert lib.nerf_amd_distortion_loss_backward(_ptr(w), _ptr(t), N, S, mode, scale, _ptr(gt), _ptr(aw[GUARD:]) if need_w else None,
                                                     _ptr(at[GUARD:]) if need_t else None, stream) == 0
        torch.cuda.synchronize()
        name = "%s ABI backward need=(%d, %d)" % (tag, need_w, need_t)
        _exact(name + " guards written", _guards_intact(aw) + _guards_intact(at))
        for need, a, want in ((need_w, aw, want_w), (need_t, at, want_t)):
            body = a[GUARD:-GUARD].view_as(want)
            if need:
                _exact(name + " differs from ops", int((~((body == want) | (torch.isnan(body) & torch.isnan(want)))).sum()))
            else:
                _exact(name + " unrequested gradient written", int((body != G.POISON).sum()))


@pytest.mark.parametrize("N,M,K", [(5, 63, 65), (5, 129, 257), (5, 682, 682), (8197, 63, 65)])
def test_interlevel_abi_guards_and_unrequested_bounds(N, M, K):
    """nerf_amd_interlevel_loss[_backward] called directly: guards around out, bounds_out and d_w_prop stay poisoned, bounds_out = NULL
    leaves its would-be buffer poisoned, and what is written equals the ops' result bit for bit"""
    from nerf_amd import ops
    from nerf_amd._lib import lib
    tag, x, g, scale = G.il_case("ties", N, M, K, False)
    w, t, w_prop, t_prop = (v.cuda() for v in x)
    gt = torch.tensor([g], device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(ops.INTERLEVEL_WORKSPACE_FLOATS, device="cuda")
    want_loss, want_b = ops.interlevel_loss(w, t, w_prop, t_prop, scale, want_bounds=True)
    want_g = ops.interlevel_loss_backward(gt.reshape(()), w, t, w_prop, t_prop, scale)
    for want_bounds in (False, True):
        out, ab = _arena(1), _arena(N * M)
        assert lib.nerf_amd_interlevel_loss(_ptr(w), _ptr(t), _ptr(w_prop), _ptr(t_prop), N, M, K, K + 1, scale, _ptr(out[GUARD:]),
                                            _ptr(ab[GUARD:]) if want_bounds else None, _ptr(ws), stream) == 0
        torch.cuda.synchronize()
        name = "%s ABI forward bounds_out=%d" % (tag, want_bounds)
        _exact(name + " guards written", _guards_intact(out) + _guards_intact(ab))
        assert torch.equal(out[GUARD], want_loss)
        body = ab[GUARD:-GUARD].view(N, M)
        _exact(name + (" differs from ops" if want_bounds else " unrequested bounds written"), int((body != (want_b if want_bounds else G.POISON)).sum()))
    ag = _arena(N * K)
    assert lib.nerf_amd_interlevel_loss_backward(_ptr(w), _ptr(t), _ptr(w_prop), _ptr(t_prop), N, M, K, K + 1, scale, _ptr(gt), _ptr(ag[GUARD:]), stream) == 0
    torch.cuda.synchronize()
    _exact(tag + " ABI backward guards written", _guards_intact(ag))
    _exact(tag + " ABI backward differs from ops", int((ag[GUARD:-GUARD].view(N, K) != want_g).sum()))


# ------------------------------------------------------------------------------------------------ the autograd modules
def test_the_autograd_modules_hand_g_and_scale_to_the_kernels():
    """Regularizer, DistortionLoss(scale) and InterlevelLoss(scale) under an upstream gradient that is not 1: loss and gradients are the
    ops' results for that g and scale, bit for bit (which the tests above hold to the specification)"""
    from nerf_amd import ops
    from nerf_amd.addtional import DistortionLoss, InterlevelLoss, Regularizer
    for gv in (0.37, -2.5):
        g = torch.tensor(gv, device="cuda")
        for mode, module, scale in ((0, Regularizer(), 1.0), (1, DistortionLoss(0.25), 0.25), (1, DistortionLoss(3.0), 3.0)):
            w, t = (v.cuda() for v in G.dist_inputs("clustered", 5, 130, mode, 21))
            wl, tl = w.clone().requires_grad_(True), t.clone().requires_grad_(True)
            loss = module(wl, tl)
            gw, gt = torch.autograd.grad(loss * g, (wl, tl))
            ew, et = ops.distortion_loss_backward(g, w, t, mode, scale)
            assert torch.equal(loss.detach(), ops.distortion_loss(w, t, mode, scale)) and torch.equal(gw, ew) and torch.equal(gt, et), (gv, mode, scale)
        for scale in (0.25, 3.0):
            w, t, w_prop, t_prop = (v.cuda() for v in G.il_inputs("ties", 5, 129, 257, True, 22))
            p = w_prop.clone().requires_grad_(True)
            loss = InterlevelLoss(scale)(w, t, p, t_prop)
            gp, = torch.autograd.grad(loss * g, p)
            assert torch.equal(loss.detach(), ops.interlevel_loss(w, t, w_prop, t_prop, scale))
            assert torch.equal(gp, ops.interlevel_loss_backward(g, w, t, w_prop, t_prop, scale)), (gv, scale)


def test_worst_ratios_on_record():
    """(runs after the tests above in file order: prints the table DESIGN.md quotes)"""
    for k in sorted(WORST):
        print("WORST %-32s MI355X %.3f   emulation %.3f" % (k, WORST[k][0], WORST[k][1]))
