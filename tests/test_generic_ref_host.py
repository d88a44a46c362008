"""The yardstick of tests/test_gpu_generic_stages.py, tested on the CPU (tests/generic_ref.py): the per-stage specifications composed into
a whole RefNeRF must equal oracle.ref_forward and its autograd gradients; the explicit adjoint formulas behind the magnitude passes must
equal torch.autograd; a torch-fp32 evaluation of every stage must stay inside its bound on every element; and the bounds must bite --
each of a list of single-term mutations of that fp32 evaluation must be reported by the comparator the GPU module uses."""
import pytest
import torch

import generic_ref as R
from oracle import nerf_oracle as O

K = R.Consts.KERNEL


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the specifications
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_ide_restatement_equals_the_oracle(deg):
    g = torch.Generator().manual_seed(deg)
    r = torch.randn(500, 3, generator=g, dtype=torch.float64)
    r = r / r.norm(dim=-1, keepdim=True) * (0.8 + 0.4 * torch.rand(500, 1, generator=g, dtype=torch.float64))
    kinv = torch.exp(torch.randn(500, 1, generator=g, dtype=torch.float64))
    want = O.ide_encode(r, kinv, deg)
    got = R.ide(r, kinv, deg)
    A = R.ide_magnitudes(r, kinv, deg)[0]
    assert float(((got - want).abs() / torch.cat((A, A), 1).clamp_min(1e-300)).max()) <= 1e-12      # relative to the terms' magnitude
    assert _rel(got, want) <= 1e-12
    # w_r along +-z: every m > 0 term is exactly zero, the m = 0 terms are att P(z) (the oracle's tensor-exponent power is NaN there)
    terms, mat = R.ide_terms(deg)
    rz = torch.tensor([[0.0, 0.0, 1.1], [0.0, 0.0, -0.9]], dtype=torch.float64)
    kz = torch.tensor([[0.5], [2.0]], dtype=torch.float64)
    out = R.ide(rz, kz, deg)
    T = len(terms)
    for t, (l, m) in enumerate(terms):
        if m > 0:
            assert float(out[:, t].abs().max()) == 0.0 and float(out[:, T + t].abs().max()) == 0.0
        else:
            want_t = torch.exp(-0.5 * l * (l + 1) * kz[:, 0]) * sum(mat[k, t] * rz[:, 2] ** k for k in range(l + 1))
            assert _rel(out[:, t], want_t) <= 1e-13 and float(out[:, T + t].abs().max()) == 0.0


@pytest.mark.parametrize("cat_origin", [True, False])
@pytest.mark.parametrize("use_srgb", [False, True])
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_composed_stages_equal_the_oracle_and_its_autograd(deg, use_srgb, cat_origin):
    Lp, hidden, bottle, M = 4, 24, 8, 96
    sd32 = O.init_linear_params(O.ref_shapes(Lp, deg, hidden, bottle, hidden, cat_origin), seed=10 + deg, std=0.25, bias_std=0.2)
    g = torch.Generator().manual_seed(100 + deg)
    pts = torch.cat((torch.rand(M, 3, generator=g, dtype=torch.float64) * 2 - 1,
                     torch.nn.functional.normalize(torch.randn(M, 3, generator=g, dtype=torch.float64), dim=-1)), dim=-1)
    cot, cot_n = torch.randn(M, 4, generator=g, dtype=torch.float64), torch.randn(M, 3, generator=g, dtype=torch.float64)
    res = []
    for fn in ("oracle", "composed"):
        sd = {k: v.double().clone().requires_grad_(True) for k, v in sd32.items()}
        p = pts.clone().requires_grad_(True)
        if fn == "oracle":
            rgbo, n = O.ref_forward(sd, p.view(1, M, 6), Lp=Lp, deg=deg, use_srgb=use_srgb, cat_origin=cat_origin)
            rgbo, n = rgbo.view(M, 4), n.view(M, 3)
        else:
            rgbo, n = R.ref_forward_composed(sd, p, Lp, deg, use_srgb, cat_origin)
        names = sorted(sd)
        grads = torch.autograd.grad((rgbo * cot).sum() + (n * cot_n).sum(), [p] + [sd[k] for k in names])
        res.append((rgbo.detach(), n.detach(), dict(zip(["pts"] + names, grads))))
    (a_o, n_o, g_o), (a_c, n_c, g_c) = res
    assert _rel(a_c, a_o) <= 1e-12 and _rel(n_c, n_o) <= 1e-12
    for k in g_o:
        assert _rel(g_c[k], g_o[k]) <= 1e-12, k


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_explicit_directional_adjoint_equals_autograd(deg):
    h, d, do, gn, _, _ = R.dir_inputs(257, deg)
    ref, _ = R.dir_backward_spec(h, d, deg, do, gn)
    got = R.dir_backward_explicit(h.double(), d.double(), deg, do.double(), gn.double())
    A = R.dir_backward_explicit(h.double(), d.double(), deg, do.double(), gn.double(), mag=True)
    assert float(((got - ref).abs() / A.clamp_min(1e-300)).max()) <= 1e-12           # (fp64 roundoff times att_depth, up to 2.4e4)
    assert bool((A >= got.abs() * (1 - 1e-12)).all())                                   # a magnitude pass dominates the value
    zero = ref[1]                                                                        # the zero normal head: -dn / eps, cden's guard gives 0
    assert bool(torch.isfinite(ref).all()) and float(zero[:3].abs().max()) > 1e5


@pytest.mark.parametrize("use_srgb", [False, True])
def test_explicit_combination_and_pe_adjoints_equal_autograd(use_srgb):
    h, s, g = R.combine_inputs(300, use_srgb)
    (d_spec, _), (d_heads, _) = R.combine_backward_spec(g, h, s, use_srgb, R.Consts.EXACT)
    e_spec, e_heads = R.combine_explicit(h.double(), s.double(), use_srgb, R.Consts.EXACT, g=g.double())
    assert _rel(e_spec, d_spec) <= 1e-12 and _rel(e_heads, d_heads) <= 1e-12
    (d_spec, _), (d_heads, _) = R.combine_backward_spec(g, h, s, use_srgb)
    # the adjoint w.r.t. the PRE-activation, by autograd through sigmoid(pre), where spec has a logit
    inner = (s > 0).all(dim=1) & (s < 1).all(dim=1)
    pre = torch.logit(s[inner].double()).requires_grad_(True)
    out = R.combine_forward(h[inner].double(), pre, use_srgb, K)
    gp, = torch.autograd.grad((out * g[inner].double()).sum(), pre)
    assert _rel(d_spec[inner], gp) <= 1e-9                                               # (logit / sigmoid round trip)
    ref, _ = R.combine_spec(h, s, use_srgb, R.Consts.EXACT)
    assert _rel(ref[inner], R.combine_forward(h[inner].double(), pre.detach(), use_srgb, R.Consts.EXACT)) <= 1e-12
    for L, cat in ((4, True), (12, False)):
        x, de = R.pe_inputs(100, L, cat)
        ref, _ = R.pe_backward_spec(de, x, L, cat)
        assert _rel(R.pe_backward_explicit(de.double(), x.double(), L, cat), ref) <= 1e-13
        enc = R.pe_forward(x.double(), L, cat)
        assert torch.equal(enc[:, (3 if cat else 0):], O.positional_encoding(x.double(), L))


# ------------------------------------------------------------------------------------------------ an fp32 evaluation stays inside every bound
def _dir_fp32(h, d, deg, do, gn):
    """the torch-fp32 evaluations of the directional stage: the kernel's order, and the specification itself with autograd"""
    out_e, n_e = R.dir_forward_explicit(h, d, deg)
    hh = h.clone().requires_grad_(True)
    out_s, n_s = R.dir_forward(hh, d, deg, K)
    g_s, = torch.autograd.grad((out_s * do).sum() + (n_s * gn).sum(), hh)
    return (out_e, n_e, R.dir_backward_explicit(h, d, deg, do, gn)), (out_s.detach(), n_s.detach(), g_s[:, [0, 1, 2, 9]])


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_fp32_directional_stage_is_inside_its_bounds(deg):
    for M in (257, 1000):
        h, d, do, gn, _, _ = R.dir_inputs(M, deg)
        ref_b, tol_b = R.dir_backward_spec(h, d, deg, do, gn)
        for out, n, gb in _dir_fp32(h, d, deg, do, gn):
            rep = R.dir_forward_check(h, d, deg, out, n)
            assert R.worst(*rep.values()) <= 1.0, (M, rep)
            rb = R.compare(gb, ref_b, tol_b)
            assert rb["worst"] <= 1.0, (M, rb)


def test_dir_backward_constant_is_four_times_the_fp32_evaluation():
    """re-measures DIR_BWD_MEASURED: the smallest C that holds the fp32 evaluations over the test's inputs.  The host's vector math
    library decides the last bit of an fp32 evaluation, so another host may measure a few per cent more than the record: 10 % is allowed
    on top of C / 4 here (the bound itself, C, is not touched by this)."""
    for deg in (1, 2, 3, 4, 5):
        m = 0.0
        for M in R.MS:
            h, d, do, gn, _, _ = R.dir_inputs(M, deg)
            for _, _, gb in _dir_fp32(h, d, deg, do, gn):
                m = max(m, R.dir_backward_measure(gb, h, d, deg, do, gn))
        print("ide_level %d: measured C %.3f (recorded %.2f), bound C %.0f" % (deg, m, R.DIR_BWD_MEASURED[deg], R.DIR_BWD_C[deg]))
        assert 4 * m <= 1.1 * R.DIR_BWD_C[deg] and 4 * max(R.DIR_BWD_MEASURED.values()) <= R.DIR_BWD_C[deg]


@pytest.mark.parametrize("use_srgb", [False, True])
def test_fp32_combination_is_inside_its_bounds(use_srgb):
    for M in (9, 257, 1000):
        h, s, g = R.combine_inputs(M, use_srgb)
        assert R.compare(R.combine_explicit(h, s, use_srgb), *R.combine_spec(h, s, use_srgb))["worst"] <= 1.0
        d_spec, d_heads = R.combine_explicit(h, s, use_srgb, g=g)
        want_spec, want_heads = R.combine_backward_spec(g, h, s, use_srgb)
        assert R.compare(d_spec, *want_spec)["worst"] <= 1.0 and R.compare(d_heads, *want_heads)["worst"] <= 1.0


def test_fp32_pe_adjoint_contraction_and_product_are_inside_their_bounds():
    for L in (4, 10, 12, 16):
        for cat in (True, False):
            x, de = R.pe_inputs(258, L, cat)
            assert R.compare(R.pe_backward_explicit(de, x, L, cat), *R.pe_backward_spec(de, x, L, cat))["worst"] <= 1.0, (L, cat)
    x, g = R.contract_inputs(1000)
    xx = x.clone().requires_grad_(True)
    out = O.contract(xx)
    pb, = torch.autograd.grad((out * g).sum(), xx)
    assert R.compare(out.detach(), *R.contract_spec(x))["worst"] <= 1.0
    assert R.compare(pb, *R.contract_spec(x, g))["worst"] <= 1.0
    gen = torch.Generator().manual_seed(1)
    for P in (1, 33, 257):
        a, b, bias = torch.randn(70, P, generator=gen), torch.randn(P, 50, generator=gen), torch.randn(50, generator=gen)
        for act, f in ((0, lambda t: t), (1, torch.relu), (2, torch.sigmoid)):
            assert R.compare(f(a @ b + bias), *R.gemm_spec(a, b, "fp32", bias, act))["worst"] <= 1.0
            q = lambda t: t.bfloat16().float()
            assert R.compare(f(q(a) @ q(b) + bias), *R.gemm_spec(a, b, "bf16", bias, act))["worst"] <= 1.0


# ------------------------------------------------------------------------------------------------ the bounds bite
def _dir_reports(h, d, deg, out, n):
    return R.worst(*R.dir_forward_check(h, d, deg, out, n).values())


@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("mut", ["imag_sign", "att", "refl2"])
def test_forward_mutations_are_reported(deg, mut):
    """(a) the sign of one imaginary term flipped, (b) one level attenuated with l l / 2, (c) the factor 2 of the reflection dropped"""
    h, d, _, _, _, _ = R.dir_inputs(257, deg)
    assert _dir_reports(h, d, deg, *R.dir_forward_explicit(h, d, deg)) <= 1.0
    assert _dir_reports(h, d, deg, *R.dir_forward_explicit(h, d, deg, mut=(mut,))) > 1.0


@pytest.mark.parametrize("deg", [1, 5])
def test_misplaced_rows_and_columns_are_reported(deg):
    """(d) row 256 replaced by row 255, on every stage's output; (e) output column T + t written to T + t + 1"""
    M, T = 257, R.T_of(deg)
    h, d, do, gn, s, g = R.dir_inputs(M, deg)
    out, n = R.dir_forward_explicit(h, d, deg)

    def row(t):
        t = t.clone(); t[256] = t[255]
        return t
    assert _dir_reports(h, d, deg, row(out), row(n)) > 1.0
    assert _dir_reports(h, d, deg, row(out), n) > 1.0 and _dir_reports(h, d, deg, out, row(n)) > 1.0
    gb = R.dir_backward_explicit(h, d, deg, do, gn)
    ref_b = R.dir_backward_spec(h, d, deg, do, gn)
    assert R.compare(gb, *ref_b)["worst"] <= 1.0 < R.compare(row(gb), *ref_b)["worst"]
    for srgb in (False, True):
        hc, sc, gc = R.combine_inputs(M, srgb)
        want = R.combine_spec(hc, sc, srgb)
        assert R.compare(row(R.combine_explicit(hc, sc, srgb)), *want)["worst"] > 1.0
        d_spec, d_heads = R.combine_explicit(hc, sc, srgb, g=gc)
        w_spec, w_heads = R.combine_backward_spec(gc, hc, sc, srgb)
        assert R.compare(row(d_spec), *w_spec)["worst"] > 1.0 and R.compare(row(d_heads), *w_heads)["worst"] > 1.0
    x, de = R.pe_inputs(M, 10, True)
    assert R.compare(row(R.pe_backward_explicit(de, x, 10, True)), *R.pe_backward_spec(de, x, 10, True))["worst"] > 1.0
    xc, gcn = R.contract_inputs(M)
    assert R.compare(row(O.contract(xc)), *R.contract_spec(xc))["worst"] > 1.0
    for t in (0, T - 2):
        shifted = out.clone()
        shifted[:, T + t + 1] = out[:, T + t]
        shifted[:, T + t] = -7.25                                                      # what the sentinel-filled buffer would keep
        assert _dir_reports(h, d, deg, shifted, n) > 1.0


@pytest.mark.parametrize("deg", [2, 3, 4, 5])
def test_adjoint_mutations_are_reported(deg):
    """(f) d_kinv without its sig factor at level l = 2 (sig = 3; ide_level 1 has the level l = 1 only, whose sig is 1)"""
    h, d, do, gn, _, _ = R.dir_inputs(257, deg)
    ref = R.dir_backward_spec(h, d, deg, do, gn)
    assert R.compare(R.dir_backward_explicit(h, d, deg, do, gn), *ref)["worst"] <= 1.0
    rep = R.compare(R.dir_backward_explicit(h, d, deg, do, gn, mut=("kinv_sig",)), *ref)
    assert rep["worst"] > 1.0 and rep["where"][1] == 3


def test_slope_side_and_octave_mutations_are_reported():
    """(g) srgb_slope taken on the wrong side of the knee for one row, (h) one octave's 2^f left out of the PE adjoint"""
    h, s, g = R.combine_inputs(257, True)
    w_spec, w_heads = R.combine_backward_spec(g, h, s, True)
    d_spec, d_heads = R.combine_explicit(h, s, True, g=g, mut=("slope_side",))
    assert R.compare(d_heads, *w_heads)["worst"] > 1.0 and R.compare(d_heads, *w_heads)["where"][0] == 0
    assert R.compare(d_spec, *w_spec)["worst"] > 1.0
    for L in (4, 16):
        x, de = R.pe_inputs(257, L, True)
        ref = R.pe_backward_spec(de, x, L, True)
        assert R.compare(R.pe_backward_explicit(de, x, L, True), *ref)["worst"] <= 1.0
        assert R.compare(R.pe_backward_explicit(de, x, L, True, mut=("octave",)), *ref)["worst"] > 1.0


def test_comparator_counts_every_element():
    ref, tol = torch.zeros(3, 2, dtype=torch.float64), torch.full((3, 2), 1e-6, dtype=torch.float64)
    assert R.compare(torch.zeros(3, 2), ref, tol)["worst"] == 0.0
    got = torch.zeros(3, 2); got[2, 1] = float("nan")
    assert R.compare(got, ref, tol) == {"worst": float("inf"), "where": (2, 1)}
    got = torch.zeros(3, 2); got[1, 0] = 1e-30
    assert R.compare(got, ref, torch.zeros(3, 2, dtype=torch.float64))["worst"] == float("inf")      # tol = 0 means bit-equal
    got = torch.zeros(3, 2); got[0, 1] = 3e-6
    rep = R.compare(got, ref, tol)
    assert abs(rep["worst"] - 3.0) < 1e-6 and rep["where"] == (0, 1)
