"""The yardstick of tests/test_gpu_sampling.py, tested on the CPU (tests/sampling_ref.py).

  * the specifications equal the oracle's (oracle/nerf_oracle.py) on the golden inputs g07 (inverse sampling, both modes, sorted and raw),
    g02 (stratified depths and points) and g08 (length2pts): the fp32 evaluation bit for bit, the fp64 values within the derived bounds;
  * the kernel's order of CDF additions -- cascade normaliser, 64-wide fp64 wave scan plus carry -- rounds to torch.cumsum's fp32 CDF on
    every input the GPU module builds (sampling_ref.assert_wave_cdf, called by every check);
  * a torch-fp32 evaluation of every entry point stays inside every bound, with zero index mismatches, on exactly the inputs the GPU
    module builds: both modules run the same check functions of sampling_ref, over sampling_ref.Emulation here and over nerf_amd.ops there;
  * the bounds bite: each planted single-term fault is reported by those same checks; the table the test prints also says which faults
    pass the OLD gates on the OLD tests' inputs;
  * the constructed rows whose raw samples descend across a boundary of the sort's 256 buckets exist, sampling_ref.EXAMPLE_ROW among them.

PLANTED FAULTS against the old gates (tests/test_gpu_parity.py: `below` equal and max |z| error <= 2e-6 on rand**3 + 0.01 weights, depths
in [2, 6], random uniforms; tests/test_gpu_ray_warp.py: 5e-6 absolute and 1 % of `below`).  "old: pass" = the old test does not see it.

    right_false         new: reported   old: pass  (no uniform of the old inputs sits on a CDF edge)
    no_eps              new: reported   old: FAIL
    clamp_moved (1e-4)  new: reported   old: pass  (the clamp never fires: every pdf value of the old inputs is above 1e-4)
    clamp_absent        new: reported   old: pass
    above_unclamped     new: reported   old: pass  (no u >= cdf[-1])
    below_unclamped     new: reported   old: pass  (no u < 0)
    pdf_from_0          new: reported   old: FAIL
    bins_from_depths    new: reported   old: FAIL
    cdf_ulp             new: reported   old: pass  (one ulp of one CDF entry moves a sample by ~1e-7 and no uniform is next to the edge)
    norm_left_to_right  new: reported   old: FAIL  (an ulp of the normaliser moves EVERY CDF entry of the row; one of 53 x 97 random uniforms falls between)
    sort_by_u           new: reported   old: pass  (ascending bins in [2, 6]: no sample leaves its bin)
    below_unsorted      new: reported   old: FAIL
    jitter_wrong_count  new: reported   (depth draws: the old parity tests compare with the oracle's own expression: FAIL there too)
    warp_no_clamp       new: reported   old: pass  (tests/test_gpu_ray_warp.py draws s inside [0, 1])

The test asserts the "new" column and the "old" column as printed (test_planted_faults_and_the_old_gates)."""
import pytest
import torch

import sampling_ref as S
from conftest import gate
from oracle import nerf_oracle as O

E = S.Emulation()
WORST = {}


def _gates(items):
    for name, value, limit in items:
        gate("host fp32 emulation: " + name, value, limit)
        key = "index" if limit == 0 else " ".join(w for w in name.split()[1:] if "=" not in w)
        WORST[key] = max(WORST.get(key, 0.0), value)


# ------------------------------------------------------------------------------------------------ the specifications against the oracle
def test_inverse_specs_equal_the_oracle_on_g07(golden):
    g = golden("g07_inverse")
    w, z, u = g["w"], g["z"], g["u"]
    v, below, _ = S.sample_eval(w, z, u, 0, True)
    assert torch.equal(v, g["z_sorted"]) and torch.equal(below, g["below_sorted"])
    assert torch.equal(S.sample_eval(w, z, u, 0, False)[0], g["z_raw"])
    mids, pw = S.make_bins(z, 0), S.make_pdf_weights(w, 0)
    v, below, above = S.sample_eval(pw, mids, g["u_pdf"], 1, False)
    assert torch.equal(v, g["s_pdf"]) and torch.equal(below, g["below_pdf"]) and torch.equal(above, g["above_pdf"])
    assert torch.equal(S.cdf32(pw), O.pdf_cdf(pw)) and torch.equal(S.assert_wave_cdf(pw), O.pdf_cdf(pw))
    # the recorded fp32 results inside the fp64 specification's bounds, the indices equal
    r = S.compare_unsorted(S.sample_ref(w, z, u, 0, False), g["z_raw"], S.sample_eval(w, z, u, 0, False)[1])
    assert r["v"] <= 1.0 and r["below"] == 0
    r = S.compare_sorted(S.sample_ref(w, z, u, 0, True), g["z_sorted"], g["below_sorted"])
    assert r == {"descents": 0, "v": r["v"], "below": 0} and r["v"] <= 1.0
    r = S.compare_unsorted(S.sample_ref(pw, mids, g["u_pdf"], 1, False), g["s_pdf"], g["below_pdf"], g["above_pdf"])
    assert r["v"] <= 1.0 and r["below"] == 0 and r["above"] == 0


def test_depth_draw_specs_equal_the_oracle_on_g02_and_g08(golden):
    g = golden("g08_assembly")
    want, tol = S.length2pts_ref(g["rays"], g["zf"])["out"]
    assert S.worst(g["l2p"], want, tol) <= 1.0
    assert torch.equal(E.length2pts(g["rays"], g["zf"]), g["l2p"])
    g = golden("g02_stratified")
    sn = int(g["render_sample_num"])
    rays = torch.cat((g["origin"][None, :].expand(g["dirs_render"].shape[0], -1), g["dirs_render"]), -1)
    ref = S.stratified_ref(rays, torch.linspace(2.0, 6.0, O.RENDER_COARSE_PNUM), g["u_render"], 4.0 / sn)
    assert S.worst(g["z_render"], *ref["z"]) <= 1.0
    assert S.worst(g["pts_render"], *ref["pts"]) <= 1.0


def test_wave_scan_emulation_is_a_scan():
    """the emulated DPP scan is an inclusive prefix sum (exact on integers), and a planted ulp in the CDF is seen by assert_wave_cdf's comparison"""
    x = torch.randint(0, 1000, (5, 64), generator=torch.Generator().manual_seed(0)).double().numpy()
    assert (S._wave_scan(x) == x.cumsum(1)).all()
    w, _ = S.case_inputs(129, 1)
    assert not torch.equal(S.cdf32(w, ("cdf_ulp",)), S.wave_scan_cdf(w))


# ------------------------------------------------------------------------------------------------ the fp32 emulation inside every bound
@pytest.mark.parametrize("nw,mode", S.CASES)
def test_emulation_inside_the_inverse_sampling_bounds(nw, mode):
    _gates(S.inverse_case_gates(E, nw, mode))


@pytest.mark.parametrize("K", S.KS)
def test_emulation_inside_the_bounds_for_every_sample_count(K):
    _gates(S.sample_count_gates(E, K))


def test_emulation_on_the_fused_shapes_and_the_cross_bucket_rows():
    for C, K in S.FUSED_SHAPES:
        _gates(S.fused_gates(E, C, K, False))
    _gates(S.fused_gates(E, *S.WARPED_SHAPE, True))
    _gates(S.cross_bucket_gates(E))


@pytest.mark.parametrize("Sn", S.DRAW_SIZES)
def test_emulation_inside_the_depth_draw_bounds(Sn):
    _gates(S.draw_gates(E, Sn))


def test_worst_ratios_on_record():
    """(runs after the tests above in file order: prints the table DESIGN.md quotes)"""
    for k in sorted(WORST):
        print("WORST fp32 emulation  %-48s %.3f" % (k, WORST[k]))


# ------------------------------------------------------------------------------------------------ the bounds bite
def _reported(mut):
    impl = S.Emulation((mut,))
    items = []
    for nw, mode in ((7, 0), (7, 1), (65, 0), (65, 1)):
        items += S.inverse_case_gates(impl, nw, mode)
    items += S.cross_bucket_gates(impl)
    return [n for n, v, l in items if not v <= l]


def _old_gate_passes(mut):
    """tests/test_gpu_parity.py test_inverse_sampling_indices_are_exact_for_every_row_length on its own inputs, the fault planted"""
    w, z, u = S.old_test_inputs()
    want_z, want_b = O.inverse_sample(w, z, u, sort=True)
    got_z, got_b, _ = S.sample_eval(w, z, u, 0, True, S.F32, (mut,))
    return bool(torch.equal(got_b, want_b)) and float((got_z.double() - want_z.double()).abs().max()) <= 2e-6


OLD_GATE_PASSES = {"right_false": True, "no_eps": False, "clamp_moved": True, "clamp_absent": True, "above_unclamped": True, "below_unclamped": True,
                   "pdf_from_0": False, "bins_from_depths": False, "cdf_ulp": True, "norm_left_to_right": False, "sort_by_u": True, "below_unsorted": False}


def test_planted_faults_and_the_old_gates():
    assert set(OLD_GATE_PASSES) == set(S.INVERSE_FAULTS)
    assert not _reported(()), "the unmutated emulation must pass"
    for mut in S.INVERSE_FAULTS:
        bad = _reported(mut)
        old = _old_gate_passes(mut)
        print("FAULT %-20s new checks: %3d gates violated (first: %s)   old 2e-6 gate on the old inputs: %s" % (mut, len(bad), bad[0] if bad else "-", "pass" if old else "FAIL"))
        assert bad, mut
        assert old == OLD_GATE_PASSES[mut], mut
    # the depth draws
    for mut in S.DRAW_FAULTS:
        bad = [n for Sn in S.DRAW_SIZES for n, v, l in S.draw_gates(S.Emulation((mut,)), Sn) if not v <= l]
        print("FAULT %-20s new checks: %3d gates violated (first: %s)" % (mut, len(bad), bad[0] if bad else "-"))
        assert bad, mut
    # W without its clamp against tests/test_gpu_ray_warp.py's 5e-6: its s are inside [0, 1], where the clamp changes nothing
    s = torch.rand(64, 64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(S.warp_eval(s, 0.2, 1000.0, ("warp_no_clamp",)), S.warp_eval(s, 0.2, 1000.0))


def test_sort_fault_needs_the_constructed_rows_on_benign_bins():
    """sorted by u instead of by value: invisible on ascending bins in [2, 6] (the old inputs), reported on the cross-bucket rows"""
    impl = S.Emulation(("sort_by_u",))
    w, z, u = S.old_test_inputs()
    res = S.compare_sorted(S.sample_ref(w, z, u, 0, True), *impl.inverse(w, z, u, 0, True)[:2])
    assert res["descents"] == 0 and res["below"] == 0 and res["v"] <= 1.0
    bad = [n for n, v, l in S.cross_bucket_gates(impl) if not v <= l]
    assert any("descents" in n for n in bad) and any("below" in n for n in bad)


# ------------------------------------------------------------------------------------------------ the cross-bucket rows
def test_cross_bucket_rows():
    w, z, u, m = S.cross_bucket_rows()
    assert w.shape[0] >= 9 and w.shape[1] == 6                  # the example and at least 8 found by the seeded search
    ex = S.EXAMPLE_ROW
    f = lambda v: torch.tensor(v, dtype=S.F32)
    assert torch.equal(w[0], f(ex["w"])) and torch.equal(z[0], f(ex["z"])) and torch.equal(u[0], f(ex["u"]))
    raw = O.inverse_sample(w, z, u, sort=False)
    assert torch.equal(raw[0], f(ex["raw"]))
    assert bool((u[:, 0] < u[:, 1]).all()) and bool((raw[:, 0] > raw[:, 1]).all())            # ascending uniforms, descending samples
    b = S.bucket_of(u)
    assert tuple(b[0].tolist()) == ex["buckets"]
    assert torch.equal(b[:, 1].long(), m) and torch.equal(b[:, 0].long(), m - 1)              # the pair straddles the boundary m / 256
    assert bool(((m & (m - 1)) != 0).all())                                                   # no power of two
    assert bool((u[:, 1].double() * 256 == m.double()).all())                                 # the edge IS the boundary
    assert bool((z[:, 1:] >= z[:, :-1]).all())                                                # ascending bins: the bucket path
    zs, bs = O.inverse_sample(w, z, u, sort=True)
    _, braw, _ = O.sample_pdf(S.make_bins(z, 0), S.make_pdf_weights(w, 0), u)
    assert torch.equal(bs, torch.flip(braw, (-1,))) and bool((braw[:, 0] < braw[:, 1]).all())  # torch.sort swaps `below` with the values
