"""The yardstick of tests/test_gpu_update.py, tested on the CPU (tests/update_ref.py).

  * a torch-fp32 emulation of bwd_launch_adam + adam_kernel (counter, tables of 48, the element loop's operation list) stays inside every
    bound, with every guard element and the counter exact, on exactly the inputs the GPU module builds: both modules run the same check
    functions of update_ref, over update_ref.Emulation here and over nerf_amd.ops.adam_step there;
  * the specification's scalars and one step of it equal torch.optim.Adam's (fp64 parameters, torch's own single-tensor rule);
  * the bounds bite: each planted fault is reported by those same checks under the default betas; the table the test prints says by which
    gate, and in which value regime a fault shows when it does not show in all five;
  * the clipping comparator passes both of torch's implementations on synthetic gradients and reports a range that escaped the scale, a
    stale range in the norm, a norm over part of the buffer and a coefficient that is not clamped.

PLANTED FAULTS.  test_planted_faults_are_reported prints, for each, the gates that report it and the value regimes (generic, fresh, g=0,
tiny, cancelling) in which it leaves an output outside its bound.  No fault shows in one regime alone: parameters at exactly zero make
p' the bare update, where a relative change of the denominator of 1e-7 is already outside the bound.  What does NOT show:

    scale_not_squared       nothing at grad_scale 1, and nothing in the g=0 regime at any scale (v' through it p'; m' is right)
    lerp_beta1              nothing at beta1 = 0.5, where the two weights coincide: the default betas carry it (m' and p')
    old_m                   m' and v' are right, p' alone reports it
    tensor_48_skipped       needs 49 tensors or more;  tensor_47_twice 48 or more;  counter_per_launch 49 or more (the counter reads
                            t0 + 2, and the second table's p' is formed with the next step's bias corrections)
    tail_untouched          only the last n mod 256 elements of each tensor differ
    bias_correction_at_t0   at t0 = 0 both corrections are 0 and p' is not finite; eps_before_division and eps_in_sqrt move the
                            denominator by eps (1 / bc2_sqrt - 1) and by up to sqrt(eps): every regime"""
import pytest
import torch

import update_ref as R
from conftest import gate

E = R.Emulation()
WORST = {}


def _gates(items):
    for name, value, limit in items:
        gate("host fp32 emulation: " + name, value, limit)
        key = "exact" if limit == 0 else name.split()[-1] if name.startswith("update adam") else name
        WORST[key] = max(WORST.get(key, 0.0), value)


# ------------------------------------------------------------------------------------------------ the specification is torch's
@pytest.mark.parametrize("si", range(len(R.SCALARS)))
def test_specification_equals_torch_adam_in_fp64(si):
    """t0 steps of torch.optim.Adam are not needed: its step counter is state.  One step of torch's single-tensor rule on fp64 tensors
    from (p, m, v, step = t0) equals the fp64 specification evaluated with DOUBLE scalars to fp64 rounding, and the fp32 scalars of
    kernel_scalars are those doubles rounded once."""
    t0, lr, b1, b2, eps = R.SCALARS[si]
    tab = R.table(47)
    sel = tab.mask & (tab.regime != 3)                         # (the tiny regime's p' moves by 1e-16 relative: nothing an fp64 comparison of two associations resolves)
    p, g, m, v = (x[sel].double() for x in (tab.p, tab.g, tab.m, tab.v))
    par = torch.nn.Parameter(p.clone())
    par.grad = g.clone()
    opt = torch.optim.Adam([par], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[par] = {"step": torch.tensor(float(t0)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    t = t0 + 1
    sc64 = {"step_size": lr / (1 - b1 ** t), "bc2_sqrt": (1 - b2 ** t) ** 0.5, "w1": 1 - b1, "w2": 1 - b2, "b2": b2, "eps": eps, "gs": 1.0}
    st = opt.state[par]
    assert float(st["step"]) == t
    # two fp64 evaluations of the same operation list (torch associates lerp and addcdiv its own way, with as many roundings): each is
    # within the fp32 bound scaled from u = 2^-24 to 2^-53 of the exact value
    ref = R.adam_ref(p, g, m, v, sc64)
    for got, k in ((par.data, "p"), (st["exp_avg"], "m"), (st["exp_avg_sq"], "v")):
        assert R.worst(got, ref[k][0], 2.0 * 2.0 ** -29 * ref[k][1]) <= 1.0, k
    sc = R.kernel_scalars(t, lr, b1, b2, eps)
    for k in ("step_size", "bc2_sqrt", "w1", "w2", "b2", "eps"):
        assert sc[k] == R.f32c(sc64[k]) and abs(sc[k] - sc64[k]) <= R.U * abs(sc64[k])


def test_table_layout():
    """odd offsets, a guard on both sides of every view, every regime at every length, every length on both sides of the 47 / 48 seam"""
    tab = R.table(97)
    assert len(tab.ranges) == 97 and all(o % 2 == 1 for o, _ in tab.ranges)
    for o, n in tab.ranges:
        assert not tab.mask[o - 1] and not tab.mask[o + n] and bool(tab.mask[o:o + n].all())
    assert {n for _, n in tab.ranges[37:48]} == set(R.LENGTHS) == {n for _, n in tab.ranges[48:59]}
    seen = {(n, int(r)) for (o, n) in tab.ranges for r in tab.regime[o:o + n].unique()}
    assert seen == {(n, r) for n in R.LENGTHS for r in range(len(R.REGIMES))}
    assert max(R.LENGTHS) > 3 * R.GRID_PASS and (max(R.LENGTHS) % R.GRID_PASS) % 256 != 0     # a third pass of the grid with a ragged tail
    tiny = tab.mask & (tab.regime == 3)
    assert float(tab.v[tiny].min()) < 2.0 ** -126 and float((tab.g[tiny] * tab.g[tiny]).min()) == 0.0       # subnormal v, g^2 underflows
    assert R.kernel_cases()[0] == (1, 0, 1.0) and len(R.kernel_cases()) == 28
    assert {(c, si) for c, si, _ in R.kernel_cases()} == {(c, si) for c in R.COUNTS for si in range(4)}
    assert {(si, gs) for c, si, gs in R.kernel_cases() if c == 49} == {(si, gs) for si in range(4) for gs in R.GRAD_SCALES}


# ------------------------------------------------------------------------------------------------ the fp32 emulation inside every bound
@pytest.mark.parametrize("count,si,gs", R.kernel_cases())
def test_emulation_inside_the_adam_bounds(count, si, gs):
    _gates(R.kernel_case_gates(E, count, si, gs))


def test_emulation_at_the_counters_end():
    _gates(R.counter_end_gates(E))


def test_emulation_of_the_class_trajectory():
    params, grads = R.class_inputs()
    _gates(R.class_gates(R.emulate_class(params, grads), R.class_reference(params, grads)))


def test_worst_ratios_on_record():
    """(runs after the tests above in file order: prints the table DESIGN.md quotes)"""
    for k in sorted(WORST):
        print("WORST fp32 emulation  %-72s %.3f" % (k, WORST[k]))


# ------------------------------------------------------------------------------------------------ the bounds bite
FAULT_CASES = ((49, 0, 1.0), (49, 1, 0.5), (49, 2, 1.0 / 3.0), (97, 1, 1.0))          # default betas only


def _reported(mut):
    impl = R.Emulation((mut,) if mut else ())
    items = []
    for count, si, gs in FAULT_CASES:
        items += R.kernel_case_gates(impl, count, si, gs)
    return [n for n, v, l in items if not v <= l]


def _regimes_seen(mut, count=49, si=1, gs=0.5):
    """the value regimes in which the fault leaves any output outside its bound (one call, default betas)"""
    tab = R.table(count)
    t0, lr, b1, b2, eps = R.SCALARS[si]
    state = (tab.p, tab.m, tab.v)
    out = R.Emulation((mut,)).adam(tab, state, t0, lr, b1, b2, eps, gs)
    ref = R.adam_ref(tab.p, tab.g, tab.m, tab.v, R.kernel_scalars(t0 + 1, lr, b1, b2, eps, gs))
    seen = []
    for r, name in enumerate(R.REGIMES):
        sel = tab.mask & (tab.regime == r)
        if any(R.worst(got[sel], ref[k][0][sel], ref[k][1][sel]) > 1.0 for k, got in (("p", out[0]), ("m", out[1]), ("v", out[2]))):
            seen.append(name)
    return seen


def test_planted_faults_are_reported():
    assert not _reported(None), "the unmutated emulation must pass"
    for mut in R.ADAM_FAULTS:
        bad = _reported(mut)
        seen = _regimes_seen(mut)
        print("FAULT %-24s %3d gates violated (first: %s)   regimes: %s" % (mut, len(bad), bad[0] if bad else "-", ", ".join(seen) if seen else "-"))
        assert bad, mut
    # the class trajectory sees the element-level faults too
    params, grads = R.class_inputs()
    ref = R.class_reference(params, grads)
    for mut in R.ELEMENT_FAULTS:
        assert any(not v <= l for _, v, l in R.class_gates(R.emulate_class(params, grads, (mut,)), ref)), mut


def test_fault_visibility_by_regime_and_scalar_set():
    """what the docstring says about where a fault does NOT show"""
    assert set(_regimes_seen("scale_not_squared")) == set(R.REGIMES) - {"g=0"}
    assert not _regimes_seen("scale_not_squared", gs=1.0)
    for mut in ("bias_correction_at_t0", "eps_before_division", "eps_in_sqrt", "lerp_beta1", "old_m"):
        assert set(_regimes_seen(mut)) == set(R.REGIMES), mut
    # beta1 = 0.5: the lerp fault is invisible -- the reason that scalar set is not the only one
    assert all(v <= l for _, v, l in R.kernel_case_gates(R.Emulation(("lerp_beta1",)), 49, 3, 1.0))
    # old_m: m' and v' stay right
    bad = [n for n, v, l in R.kernel_case_gates(R.Emulation(("old_m",)), 49, 1, 1.0) if not v <= l]
    assert bad and all(n.endswith("p'") for n in bad)
    # the table faults need their tensor count
    for mut, count in (("tensor_48_skipped", 48), ("tensor_47_twice", 47), ("counter_per_launch", 48)):
        assert all(v <= l for _, v, l in R.kernel_case_gates(R.Emulation((mut,)), count, 1, 1.0)), mut
    bad = [n for n, v, l in R.kernel_case_gates(R.Emulation(("counter_per_launch",)), 49, 1, 1.0) if not v <= l]
    assert any("counter" in n for n in bad) and any(n.endswith("p'") for n in bad)


# ------------------------------------------------------------------------------------------------ the clipping comparator
def _synthetic_grads():
    gn = torch.Generator().manual_seed(11)
    return [torch.randn(s, generator=gn) * sc for s, sc in (((256, 63), 1e-3), ((256,), 1e-2), ((3, 8193), 1e-5), ((1,), 1.0), ((65, 129), 1e-4))]


@pytest.mark.parametrize("flat", [True, False])
def test_clip_comparator_passes_torchs_implementations_and_reports_the_faults(flat):
    g = _synthetic_grads()
    c = 0.5 * R.norm64(g)
    tag = "update clip synthetic %s" % ("flat" if flat else "per-tensor")
    clipped = R.emulate_clip(g, c, flat)
    w1 = R.f32c(0.1)
    m = [t * w1 for t in clipped]
    v = [R.f32c(0.001) * (t * t) for t in clipped]
    _gates(R.clip_gates(tag, g, clipped, c, flat, exp_avg=m, exp_avg_sq=v, twin=[t.clone() for t in g]))
    for mut in R.CLIP_FAULTS:
        cc = 2.0 * R.norm64(g) if mut == "scale_not_clamped" else c          # (an unclamped coefficient shows when the clip is inactive)
        if not flat and mut != "range_escaped_scale":
            continue                                                          # (the other three are faults of the flat expression)
        bad = [n for n, v_, l in R.clip_gates(tag, g, R.emulate_clip(g, cc, flat, (mut,)), cc, flat) if not v_ <= l]
        print("FAULT %-28s %d gates violated (first: %s)" % (mut, len(bad), bad[0] if bad else "-"))
        assert bad, mut
    # the optimizer fed the UNCLIPPED gradients: reported by check 4
    bad = [n for n, v_, l in R.clip_gates(tag, g, clipped, c, flat, exp_avg=[t * w1 for t in g], exp_avg_sq=[R.f32c(0.001) * (t * t) for t in g]) if not v_ <= l]
    assert any("exp_avg !=" in n for n in bad) and any("exp_avg_sq" in n for n in bad)
