"""The yardstick of tests/test_gpu_regularizers.py, tested on the CPU (tests/regularizer_ref.py).

  * the `uniform` family is bit for bit the inputs of the old tests (test_gpu_distortion._inputs, interlevel_ref.make_inputs), the other
    families have the properties they are named for;
  * the distortion specification equals golden g26_regularizer (the real reference's Regularizer in fp32) within the fp32 reference's own
    error, the interlevel specification (overlap mask) equals the prefix-sum route of interlevel_ref within the prefix sums' own error;
  * the emulation -- the backward's closed forms, the two-tap scatter, the F prefix -- stays inside every bound on every family at the
    host shapes (so the closed forms equal autograd), and its worst share of each bound is printed;
  * the bounds bite: every planted single-term fault is reported; the table below also says, per fault, whether there is a case on which
    the new check reports it while the OLD norm-wise gate (1e-6 of the largest entry; one ulp of the largest bound) passes on the very
    same inputs and outputs.

PLANTED FAULTS.  Each is a single-term change of the emulation (regularizer_ref.Emulation(faults=...)).  "same inputs" = the old norm-wise
gates evaluated on a host case on which the new check reports the fault (pass: at least one such case passes every old gate); "old
tests" = the old tests as they were: their own inputs, g = 1, scale = 1, one grid-stride trip, the norm-wise gates.

    kernel      fault             what                                                          new        same inputs  old tests
    distortion  sgn0_plus         sgn(0) = +1 on tied centres                                   reported   FAIL         pass  (no tied centres)
    distortion  colM_unwritten    column M not written when M % 128 == 0                        reported   FAIL         FAIL
    distortion  no_handover       the lane-63 hand-over of dist_from_below replaced by 0        reported   FAIL         FAIL
    distortion  carry_kept        carry_w / carry_t not reset between two rays of one wave      reported   FAIL         pass  (no second trip in mode 0)
    distortion  q_term_w          mode 0: a_i taken as w_i in the Q term                        reported   FAIL         FAIL
    distortion  third_dropped_dt  the 1/3 of cQ dropped in d/dt                                 reported   FAIL         FAIL
    distortion  uq_fp32           u, q rounded to fp32 before pass 2 (the retired version)      reported   pass         pass
    distortion  pair_sums_fp32    D_k accumulated in fp32                                       reported   pass         pass
    distortion  g_one             g taken as 1                                                  reported   FAIL         pass  (g is always 1)
    distortion  scale_twice       scale applied twice in the backward                           reported   FAIL         pass  (scale is always 1)
    interlevel  g_one             g taken as 1                                                  reported   FAIL         pass  (g is always 1)
    interlevel  scale_twice       scale applied twice in the backward                           reported   FAIL         FAIL  (scale 0.5 at M = 64)
    interlevel  lo_unclamped      lo not clamped at 0                                           reported   FAIL         FAIL
    interlevel  hi_count_lt       count_le taken as count_lt for hi on tied edges               reported   FAIL         FAIL  (its `ties` option)
    interlevel  open_last_depth   the open form's +inf edge replaced by the last depth          reported   FAIL         FAIL
    interlevel  F_carry_dropped   the F prefix carry dropped at a 64-lane block                 reported   FAIL         FAIL
    interlevel  no_eps            the 1e-8 dropped from the denominator                         reported   pass         FAIL
    interlevel  cprefix_fp32      the w_prop prefix sum formed in fp32                          reported   pass         FAIL  (at 1024 columns only)
    interlevel  F_prefix_fp32     the F prefix sum formed in fp32                               reported   pass         FAIL  (at 1024 columns only)

Five pass the old gates on the very inputs on which the new check reports them, seven pass the old tests."""
import pytest
import torch

import interlevel_ref as R
import regularizer_ref as G
from conftest import gate

E = G.Emulation()
WORST = {}
_REFS = {}


def _dist(family, S, mode, N=5):
    key = ("d", family, S, mode, N)
    if key not in _REFS:
        tag, (w, t), g, scale = G.dist_case(family, N, S, mode)
        _REFS[key] = (tag, (w, t), g, scale, G.dist_ref(w, t, mode, g, scale))
    return _REFS[key]


def _il(family, M, K, open_form, N=5):
    key = ("i", family, M, K, open_form, N)
    if key not in _REFS:
        tag, x, g, scale = G.il_case(family, N, M, K, open_form)
        _REFS[key] = (tag, x, g, scale, G.il_ref(*x, g, scale))
    return _REFS[key]


def _gates(items, kind):
    for name, value, limit in items:
        gate("host emulation: " + name, value, limit)
        if limit:
            key = kind + " " + name.split()[-1]
            WORST[key] = max(WORST.get(key, 0.0), value)


# ------------------------------------------------------------------------------------------------ the generator
def test_uniform_family_is_the_old_tests_inputs():
    from test_gpu_distortion import _inputs
    for mode in (0, 1):
        for a, b in zip(G.old_dist_inputs(5, 65, mode, 1234), _inputs(5, 65, mode, 1234)):
            assert torch.equal(a, b)
        assert all(torch.equal(a, b) for a, b in zip(G.dist_inputs("uniform", 5, 65, mode, 77), _inputs(5, 65, mode, 77)))
    for open_form in (False, True):
        for a, b in zip(G.il_inputs("uniform", 5, 63, 65, open_form, 9), R.make_inputs(5, 63, 65, open_form, False, 9)):
            assert torch.equal(a, b)


def _decades(w):
    nz = w[w > 0]
    return float(torch.log10(nz.max() / nz.min()))


def test_the_families_have_the_properties_they_are_named_for():
    for mode in (0, 1):
        w, t = G.dist_inputs("peaked", 9, 257, mode, 3)
        assert _decades(w[2:]) >= 10 and bool((w[2:] == 0).any(1).all()) and int((w[0] != 0).sum()) == 1 and bool((w[1] == 0).all())
        w, t = G.dist_inputs("clustered", 9, 257, mode, 3)
        same = t[:, 1:] == t[:, :-1]
        assert bool((t[:, 1:] >= t[:, :-1]).all())
        assert bool((same.sum(1) >= 3).all()) and bool((same[:, 1:] & same[:, :-1]).any(1).all())          # a run of two and a run of three
        c = (t[:, :-1] + t[:, 1:]) / 2
        assert bool((c[:, 1:] == c[:, :-1]).any(1).all())                                                   # tied centres
        w, t = G.dist_inputs("degenerate", 5, 65, mode, 3)
        assert t.shape[0] >= 9 and bool((t[2] == t[2, 0]).all()) and not bool((t[3] == t[3, 0]).all())
    w, t = G.dist_inputs("unsorted", 9, 257, 0, 3)
    assert not bool((t[:, 1:] >= t[:, :-1]).all()) and bool((torch.sort(t, -1)[0][:, 1:] == torch.sort(t, -1)[0][:, :-1]).any(1).all())
    for open_form in (False, True):
        w, t, w_prop, t_prop = G.il_inputs("peaked", 9, 257, 129, open_form, 5)
        assert _decades(w[2:]) >= 10 and _decades(w_prop[2:]) >= 10 and bool((w[2:] == 0).any()) and int((w[0] != 0).sum()) == 1
        assert bool((w[1] == 0).all()) and bool((w_prop[1] == 0).all())
        assert float((w[2:].double().sum(1) - 1).abs().max()) <= 1e-6 and float((w_prop[2:].double().sum(1) - 1).abs().max()) <= 1e-6
        w, t, w_prop, t_prop = G.il_inputs("ties", 9, 129, 65, open_form, 5)
        assert bool((t[:, 1:] >= t[:, :-1]).all()) and bool((t_prop[:, 1:] >= t_prop[:, :-1]).all())
        assert bool((t[:, 0] < t_prop[:, 0]).all()) and bool((t[:, -1] > t_prop[:, -1]).all())
        hits = (t[:, :, None] == t_prop[:, None, :]).any(1).sum(1)
        assert bool((hits >= 16).all())                                                                     # fine edges that ARE proposal edges


# ------------------------------------------------------------------------------------------------ the specifications
@pytest.mark.parametrize("case", ["pipe", "unsort", "nan", "s257"])
def test_distortion_specification_equals_g26(golden, case):
    """the real reference's Regularizer, recorded in fp32: an M-term fp32 sum in the forward and another in the backward leave up to
    4 M u of the largest entry of a tensor (M u each way, twice for the norm in the denominator); the specification is inside that"""
    g = golden("g26_regularizer")
    w, t = g[case + "_w"], g[case + "_t"]
    ref = G.dist_ref(w, t, 0)
    if case == "nan":
        assert bool(torch.isnan(ref["loss"][0])) and bool(torch.isnan(ref["d_w"][0]).all()) and bool(torch.isnan(ref["d_t"][0]).all())
        assert bool(torch.isnan(g[case + "_gw"]).all()) and bool(torch.isnan(g[case + "_gt"]).all())
        return
    lim = 4 * (t.shape[1] - 1) * G.U
    gate("regularizer spec vs g26 %s loss (rel)" % case, abs(ref["loss"][0].item() - float(g[case + "_loss"])) / abs(ref["loss"][0].item()), lim)
    gate("regularizer spec vs g26 %s d/dw (of the largest entry)" % case, G._old_rel(g[case + "_gw"], ref["d_w"][0]), lim)
    gate("regularizer spec vs g26 %s d/dt (of the largest entry)" % case, G._old_rel(g[case + "_gt"], ref["d_t"][0]), lim)


@pytest.mark.parametrize("family", G.IL_FAMILIES)
def test_interlevel_specification_equals_the_prefix_sum_route(family):
    """the overlap-mask sums against interlevel_ref.evaluate (cumsum + searchsorted, autograd): equal within the sequential prefix sums'
    own error, K eps of the row's total weight for each of the two prefix entries of a bound, and the same through the gradient"""
    for M, K in ((3, 64), (63, 65), (128, 64)):
        for open_form in (False, True):
            tag, x, g, scale, ref = _il(family, M, K, open_form)
            b, loss, grad = R.evaluate(*x, scale=G.f32c(scale))
            tot = x[2].double().abs().sum(1, keepdim=True)
            assert bool(((b - ref["bounds"][0]).abs() <= 2 * K * G.EPS64 * tot).all()), tag
            assert abs(loss - ref["loss"][0].item()) <= 1e-12 * abs(loss) + 1e-300, tag
            fsum = (2 * torch.relu(x[0].double() - b) / (x[0].double() + R.EPS)).sum(1, keepdim=True) + 1e-300
            assert bool(((grad * float(torch.tensor(g, dtype=torch.float32)) - ref["d_w_prop"][0]).abs() <= 1e-11 * abs(g * scale) * fsum).all()), tag
            exact = R.evaluate(*x, scale=G.f32c(scale), bounds_fn=R.brute_bounds)
            assert torch.equal(exact[0], ref["bounds"][0]), tag


def test_wave_prefix_is_a_prefix_sum():
    x = torch.randint(0, 1000, (5, 200), generator=torch.Generator().manual_seed(0)).double()
    assert torch.equal(G.wave_prefix(x), G._excl(x))
    assert not torch.equal(G.wave_prefix(x, drop_carry=True), G._excl(x))


# ------------------------------------------------------------------------------------------------ the emulation inside every bound
@pytest.mark.parametrize("S", G.HOST_S)
@pytest.mark.parametrize("mode", [0, 1])
def test_distortion_emulation_inside_the_bounds(mode, S):
    for family in G.DIST_FAMILIES[mode]:
        tag, (w, t), g, scale, ref = _dist(family, S, mode)
        _gates(G.compare(tag, G.run_dist(E, w, t, mode, g, scale), ref), "distortion mode %d" % mode)


@pytest.mark.parametrize("M,K", G.HOST_IL_SHAPES)
def test_interlevel_emulation_inside_the_bounds(M, K):
    for family in G.IL_FAMILIES:
        for open_form in (False, True):
            tag, x, g, scale, ref = _il(family, M, K, open_form)
            _gates(G.compare(tag, G.run_il(E, x, g, scale), ref), "interlevel")


def test_degenerate_ray_keeps_its_nan_to_itself():
    """mode 0: ray 2's gradient rows and the loss are NaN in the specification, every other ray's are finite (the emulation is held to
    exactly that pattern by worst()); mode 1: ray 2's weight gradient is exact zeros and everything is finite"""
    tag, (w, t), g, scale, ref = _dist("degenerate", 65, 0)
    for k in ("d_w", "d_t"):
        nan = torch.isnan(ref[k][0])
        assert bool(nan[2].all()) and int(nan.sum()) == nan.shape[1]
        assert bool(torch.isfinite(ref[k][1][~nan]).all())
    assert bool(torch.isnan(ref["loss"][0]))
    tag, (w, t), g, scale, ref = _dist("degenerate", 65, 1)
    got = G.run_dist(E, w, t, 1, g, scale)
    assert bool((ref["d_w"][0][2] == 0).all()) and bool((ref["d_w"][1][2] == 0).all()) and bool((got["d_w"][2] == 0).all())
    assert bool(torch.isfinite(ref["d_t"][0]).all())                                 # (d/dt keeps the widths' part, kQ a^2)
    assert G.worst(torch.zeros(3), torch.tensor([0.0, float("nan"), 0.0]), torch.ones(3)) == G.INF
    assert G.worst(torch.tensor([0.0, float("nan"), 1e-3]), torch.tensor([0.0, float("nan"), 0.0]), torch.tensor([0.0, 0.0, 1e-2])) == pytest.approx(0.1)


def test_worst_ratios_on_record():
    """(runs after the tests above in file order: prints the table DESIGN.md quotes)"""
    for k in sorted(WORST):
        print("WORST host emulation  %-40s %.3f" % (k, WORST[k]))


# ------------------------------------------------------------------------------------------------ the bounds bite
# (kind, fault) -> (the old gates pass on a case that the new check reports, the old tests' own data and gates let it through)
OLD_GATE_PASSES = {
    ("distortion", "sgn0_plus"): (False, True), ("distortion", "colM_unwritten"): (False, False), ("distortion", "no_handover"): (False, False),
    ("distortion", "carry_kept"): (False, True), ("distortion", "q_term_w"): (False, False), ("distortion", "third_dropped_dt"): (False, False),
    ("distortion", "uq_fp32"): (True, True), ("distortion", "pair_sums_fp32"): (True, True), ("distortion", "g_one"): (False, True),
    ("distortion", "scale_twice"): (False, True),
    ("interlevel", "g_one"): (False, True), ("interlevel", "scale_twice"): (False, False), ("interlevel", "lo_unclamped"): (False, False),
    ("interlevel", "hi_count_lt"): (False, False), ("interlevel", "open_last_depth"): (False, False), ("interlevel", "F_carry_dropped"): (False, False),
    ("interlevel", "no_eps"): (True, False), ("interlevel", "cprefix_fp32"): (True, False), ("interlevel", "F_prefix_fp32"): (True, False)}


def _dist_cases():
    for mode in (0, 1):
        for family in G.DIST_FAMILIES[mode]:
            for S in G.HOST_S:
                yield mode, _dist(family, S, mode)


def _il_cases():
    for M, K in G.HOST_IL_SHAPES:
        for family in G.IL_FAMILIES:
            for open_form in (False, True):
                yield _il(family, M, K, open_form)


def _fault_row(kind, fault):
    """-> (cases on which the new check reports the fault, how many of those pass every old gate, a witness of either kind)"""
    impl = G.Emulation((fault,))
    reported, old_pass, witness = 0, 0, None
    if kind == "distortion":
        runs = ((tag, ref, (lambda w=w, t=t, mode=mode, g=g, scale=scale: G.run_dist(impl, w, t, mode, g, scale)))
                for mode, (tag, (w, t), g, scale, ref) in _dist_cases())
    else:
        runs = ((tag, ref, (lambda x=x, g=g, scale=scale: G.run_il(impl, x, g, scale))) for tag, x, g, scale, ref in _il_cases())
    for tag, ref, run in runs:
        got = run()
        if all(v <= l for _, v, l in G.compare(tag, got, ref)):
            continue
        reported += 1
        if G.old_gate_passes(got, ref):
            old_pass += 1
            witness = witness if (witness and old_pass > 1) else tag
        elif witness is None:
            witness = tag
    return reported, old_pass, witness


def _old_suite_passes(kind, fault):
    """the old tests as they were: their own inputs (the `uniform` family with the old seeds; interlevel with and without its `ties`
    option), g = 1, scale = 1 (0.5 at M = 64), no ray on a second grid-stride trip, the norm-wise gates -- at the host shapes"""
    impl = G.Emulation((fault,), cap=2048)
    if kind == "distortion":
        for mode in (0, 1):
            for S in G.HOST_S:
                w, t = G.old_dist_inputs(5, S, mode, 5000 + S)
                key = ("od", mode, S)
                if key not in _REFS:
                    _REFS[key] = G.dist_ref(w, t, mode)
                if not G.old_gate_passes(G.run_dist(impl, w, t, mode, 1.0, 1.0), _REFS[key]):
                    return False
        return True
    for M, K in G.HOST_IL_SHAPES + ((64, 64),):                                      # (64, 64): where the old sweep's scale 0.5 meets a gradient
        for open_form in (False, True):
            for ties in (False, True):
                x, scale = R.make_inputs(5, M, K, open_form, ties, 5000 + 10 * M + K), 0.5 if M == 64 else 1.0
                key = ("oi", M, K, open_form, ties)
                if key not in _REFS:
                    _REFS[key] = G.il_ref(*x, 1.0, scale)
                if not G.old_gate_passes(G.run_il(impl, x, 1.0, scale), _REFS[key]):
                    return False
    return True


def test_planted_faults_and_the_old_gates():
    assert set(OLD_GATE_PASSES) == {("distortion", f) for f in G.DIST_FAULTS} | {("interlevel", f) for f in G.IL_FAULTS}
    assert len(OLD_GATE_PASSES) >= 14
    for mode, (tag, (w, t), g, scale, ref) in _dist_cases():                         # the unmutated emulation passes everything, old and new
        got = G.run_dist(E, w, t, mode, g, scale)
        assert all(v <= l for _, v, l in G.compare(tag, got, ref)) and G.old_gate_passes(got, ref), tag
    for tag, x, g, scale, ref in _il_cases():
        got = G.run_il(E, x, g, scale)
        assert all(v <= l for _, v, l in G.compare(tag, got, ref)) and G.old_gate_passes(got, ref), tag
    assert _old_suite_passes("distortion", "uq_fp32") and G.Emulation().faults == ()
    same, suite = 0, 0
    for (kind, fault), (want_same, want_suite) in OLD_GATE_PASSES.items():
        reported, old_pass, witness = _fault_row(kind, fault)
        old_suite = _old_suite_passes(kind, fault)
        print("FAULT %-10s %-17s new: reported on %3d cases | old gates on the same inputs: pass on %3d of them (%s: %s) | the old tests: %s"
              % (kind, fault, reported, old_pass, "e.g." if old_pass else "first reported", witness, "pass" if old_suite else "FAIL"))
        assert reported > 0, (kind, fault)
        assert (old_pass > 0) == want_same and old_suite == want_suite, (kind, fault, old_pass, old_suite)
        same, suite = same + (old_pass > 0), suite + old_suite
    print("FAULTS %d planted, all reported; %d pass the old gates on the same inputs, %d pass the old tests" % (len(OLD_GATE_PASSES), same, suite))
    assert same >= 5
