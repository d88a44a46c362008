"""The yardstick of tests/test_gpu_ref_forward_layers.py, tested on the CPU (tests/ref_forward_ref.py, tests/forward_ref.py): the index
maps of the Ref-NeRF layout tile the stream exactly once, the unpacker inverts a Python packer written from the same header (IDE table
included), an honest emulation of ref_kernel -- fp32 chains, round-to-nearest bf16, the element-wise expressions operation by operation
in fp32 -- sits inside every bound, and each of eleven planted faults is reported by the stage it belongs to.  A fault is planted in the
emulated dump, never in repository code."""
import pytest
import torch

import backward_ref as R
import forward_ref as F
import ref_forward_ref as RR
import weights as W
from nerf_amd.ref_func import ide_table
from oracle import nerf_oracle as O

M = 64
LAY = F.LAYOUTS["ref"]
TABLE = ide_table(4)
MATRIX = [s[0] for s in RR.STAGES]
ALL = set(MATRIX) | set(RR.ELEMENTWISE) | set(RR.EXACT)


def _state(tag):
    return RR.varied_state() if tag == "varied" else W.ref_state(tag)


_BLOBS = {}


def _operands(tag, prec):
    if (tag, prec) not in _BLOBS:
        ws, bs = RR.kernel_tensors(_state(tag), TABLE)
        mats, biases = F.layer_masters(LAY, ws, bs)
        _BLOBS[(tag, prec)] = (mats, biases, F.unpack(F.pack(LAY, prec, mats, biases, ide=TABLE), LAY, prec))
    return _BLOBS[(tag, prec)]


def inputs(n, seed, wide=False):
    """positions N(0, 1.5) and unit directions; wide: every other position x 4 (outside the unit ball, where the contraction acts), the
    others x 1/4 (mostly inside), and sample 0 on the unit sphere to within rounding (the branch of the contraction is then either)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=gen) * 1.5
    if wide:
        x = x * torch.where(torch.arange(n) % 2 == 1, 4.0, 0.25)[:, None]
        x[0] = torch.tensor([0.6, 0.8, 0.0])
    d = torch.randn(n, 3, generator=gen)
    return torch.cat((x, d / d.norm(dim=1, keepdim=True)), -1)


def _noise(n, seed=9):
    return torch.randn(n, 128, generator=torch.Generator().manual_seed(seed)) * 0.1


def _run(prec, tag="he", flags=0, noise=None, contract=False, **fault):
    u = _operands(tag, prec)[2]
    pts = inputs(M, 11, wide=contract)
    run = RR.emulate(prec, u, pts, noise, flags, contract, **fault)
    return u, pts, run


def _check(prec, u, pts, run, flags=0, noise=None, contract=False):
    return RR.check_forward(prec, u, run, pts, noise, flags, contract)


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_index_map_is_a_bijection(prec):
    assert F.map_is_bijection(LAY, prec)
    assert all(LAY.START[l] + LAY.NKG[l] * LAY.NFB[l] == (LAY.START[l + 1] if l + 1 < LAY.N_LAYERS else LAY.USED_FRAGS) for l in range(LAY.N_LAYERS))
    assert all(LAY.BIAS_OFF[l] + 32 * LAY.NFB[l] == (LAY.BIAS_OFF[l + 1] if l + 1 < LAY.N_LAYERS else LAY.N_BIAS) for l in range(LAY.N_LAYERS))
    assert LAY.N_LAYERS == 18 and LAY.N_FRAGS == 2128 and LAY.N_BIAS == 4288 and LAY.N_IDE == 176
    assert LAY.packed_bytes(prec) == 2128 * (1024 if prec == "bf16" else 2048) + (4288 + 176) * 4


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_unpacker_inverts_the_python_packer(prec):
    mats, biases, u = _operands("he", prec)
    for l in range(LAY.N_LAYERS):
        assert mats[l].shape == (LAY.rows[l], LAY.in_f[l])
        assert torch.equal(u.w[l].double(), R.operand(mats[l], prec)), (prec, l)
        assert u.pad[l].numel() == 512 * LAY.NKG[l] * LAY.NFB[l] - LAY.rows[l] * LAY.in_f[l] and not bool((u.pad[l] != 0).any())
        assert torch.equal(u.b[l], biases[l]) and not bool((u.bpad[l] != 0).any())
    assert u.tail.numel() == 0 and torch.equal(u.ide, TABLE)
    # slips the round trip alone could hide (packer and unpacker share slot_column), spelled out from mlp_layout.h:
    pos, row, col = F.index_map(LAY, 13, prec)                        # D4: K groups 0..7 bottle-neck, 8..10 IDE, 11..26 hidden
    frag = lambda kg: col[2 * kg * 512: 2 * kg * 512 + 512]          # fragment (fb 0, kg) of the first block pair
    assert int(frag(7).min()) >= 112 and int(frag(7).max()) < 128
    assert set(frag(8).tolist()) == set(range(128, 136)) | set(range(147, 155))            # real 0..7 | imag 0..7
    assert set(frag(10).tolist()) == {144, 145, 146, 163, 164, 165, 166, -1}               # real 16..18, imag 16..18, n.d, padding
    assert int(frag(11).min()) == 167 and int(frag(26).max()) == 422
    assert F.ide_slot_column(19, 0) == 38 and F.ide_slot_column(19, 1) == -1 and F.ide_slot_column(20, 0) == -1
    # the head rows of H follow the 128 bottle-neck rows in the order nerf_amd.h documents: normal, roughness, diffuse, density, tint
    sd = W.ref_state("he")
    assert torch.equal(mats[8][128:131], sd["norm_col_tint_head.weight"][0:3]) and torch.equal(mats[8][131], sd["rho_tau_head.weight"][0])
    assert torch.equal(mats[8][132:135], sd["norm_col_tint_head.weight"][3:6]) and torch.equal(mats[8][135], sd["rho_tau_head.weight"][1])
    assert torch.equal(mats[8][136:139], sd["norm_col_tint_head.weight"][6:9])


def test_slot8_maps_are_bijections_and_round_trip():
    assert sorted(c for c in RR.IDE_COL if c >= 0) == list(range(39)) and RR.IDE_COL.count(-1) == 9
    assert sorted(c for c in RR.PE_COL if c >= 0) == list(range(63)) and RR.PE_COL.count(-1) == 1
    gen = torch.Generator().manual_seed(1)
    bn, ide, ex = torch.randn(5, 128, generator=gen), torch.randn(5, 39, generator=gen), torch.randn(5, 63, generator=gen)
    b2, i2, e2 = RR.split_slot8(RR.join_slot8(bn, ide, ex))
    assert torch.equal(b2, bn) and torch.equal(i2, ide) and torch.equal(e2, ex)


# ------------------------------------------------------------------------------------------------ the honest emulation
@pytest.mark.parametrize("flags", [0, RR.REF_SRGB])
@pytest.mark.parametrize("tag", ["small", "he", "varied"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_honest_emulation_is_inside_every_bound(prec, tag, flags):
    for noise in (None, _noise(M)):
        u, pts, run = _run(prec, tag, flags, noise)
        rep = _check(prec, u, pts, run, flags, noise)
        RR.assert_forward("honest %s %s flags %d" % (prec, tag, flags), rep)
        assert set(rep) == ALL
        if prec == "bf16":
            r = RR.ratios(rep)
            assert max(r["S1"], r["D2"], r["bottleneck"]) > 0.5                     # round-to-nearest attains its term: no slack to hide in


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_honest_contracted_emulation_is_inside_every_bound(prec):
    u, pts, run = _run(prec, "he", contract=True)
    assert float(pts[:, :3].norm(dim=1).min()) < 1.0 < float(pts[:, :3].norm(dim=1).max())
    RR.assert_forward("honest contracted " + prec, _check(prec, u, pts, run, contract=True))
    assert "position" in RR.failing(_check(prec, u, pts, run, contract=False))      # ... and the flag matters to the comparator


def test_the_emulation_computes_what_the_oracle_computes():
    """the emulation is the kernel's arithmetic, the oracle the reference's: same function (fp32, so to a few 1e-6), for both flags"""
    pts = inputs(200, 3)
    for tag in ("small", "he", "varied"):
        for flags in (0, RR.REF_SRGB):
            run = RR.emulate("fp32", _operands(tag, "fp32")[2], pts, None, flags)
            rgbo, normal = O.ref_forward({k: v.double() for k, v in _state(tag).items()}, pts[None].double(), use_srgb=bool(flags))
            assert float((rgbo[0] - run["rgbo"]).abs().max()) < 2e-5 and float((normal[0] - run["normal"]).abs().max()) < 2e-5, (tag, flags)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_the_varied_set_covers_the_elementwise_ranges(prec):
    """the premise of the GPU test's coverage assertion, checked here first (1000 samples of the GPU test's M = 1000 inputs)"""
    pts = inputs(1000, 1000 + 1000 % 997)
    run = RR.emulate(prec, _operands("varied", prec)[2], pts)
    cov = RR.coverage(run["aux"])
    assert all(cov.values()), [k for k, v in cov.items() if not v]
    on7, on16 = (run["acts"][7] > 0).float().mean(0), (run["acts"][16] > 0).float().mean(0)
    assert all(0.3 < float(on7[j]) < 0.7 for j in RR.UNITS7) and all(0.3 < float(on16[j]) < 0.7 for j in RR.UNITS16)
    # and the oracle agrees on what these heads do: its normal is the bias direction for the samples whose unit is off
    off = run["acts"][7][:, RR.UNITS7[0]] == 0
    _, normal = O.ref_forward({k: v.double() for k, v in _state("varied").items()}, pts[None].double())
    if prec == "fp32":
        n0 = torch.tensor([2e-7, -1e-7, 3e-7], dtype=torch.float64)
        want = -n0 / (n0.norm() + 1e-7)
        assert int(off.sum()) > 100 and float((normal[0][off] - want).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ the eleven planted faults
def _only(rep, *stages):
    bad = RR.failing(rep)
    assert set(stages) <= set(bad), (stages, bad, {k: RR.ratios(rep)[k] for k in stages})
    return bad


def test_fault_01_a_truncating_bf16_conversion_in_one_hidden_slot():
    for at in ("S2", "D5"):
        u, pts, run = _run("bf16", fault="trunc", at=at)
        assert _only(_check("bf16", u, pts, run), at) == [at]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_02_a_stale_stash_k_group_in_d4(prec):
    u, pts, run = _run(prec, fault="stale", at="D4")
    assert _only(_check(prec, u, pts, run), "D4") == ["D4"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_03_the_l4_attenuation_with_sigma_6(prec):
    u, pts, run = _run(prec, "varied", fault="sigma4")
    rep = _check(prec, u, pts, run)
    assert _only(rep, "ide") == ["ide"]
    f = rep["ide"]["where"][1] - 128
    assert RR.TL[RR.IDE_COL[f] % 19] == 4                                           # ... at a term of band l = 4


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_04_real_and_imaginary_parts_of_one_term_swapped(prec):
    u, pts, run = _run(prec, fault="reim")
    rep = _check(prec, u, pts, run)
    assert _only(rep, "ide") == ["ide"] and RR.IDE_COL[rep["ide"]["where"][1] - 128] % 19 == 7


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_05_n_dot_d_moved_to_slot_20(prec):
    u, pts, run = _run(prec, fault="ndot20")
    rep = _check(prec, u, pts, run)
    bad = _only(rep, "ndot", "ide")                                                 # the slot is empty, and a padding slot is not
    assert RR.ratios(rep)["ide"] == float("inf") and R.feature_slot(rep["ide"]["where"][1]) == (10, 0, 4)
    assert set(bad) <= {"ndot", "ide", "D0", "D4"}                                  # (the layers then multiply a zero where the dump says n.d)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_06_noise_with_the_two_runs_of_a_k_group_swapped(prec):
    noise = _noise(M)
    u, pts, run = _run(prec, noise=noise, fault="noiseswap")
    rep = _check(prec, u, pts, run, noise=noise)
    assert _only(rep, "bottleneck") == ["bottleneck"] and rep["bottleneck"]["where"][1] // 16 == 3


def test_fault_07_diffuse_and_tint_rows_exchanged():
    u, pts, run = _run("fp32", "varied", fault="rows")
    rep = _check("fp32", u, pts, run)
    assert _only(rep, "heads") == ["heads"] and 4 <= rep["heads"]["where"][1] <= 10


def test_fault_08_the_density_taken_from_head_row_6():
    u, pts, run = _run("fp32", fault="density6")
    rep = _check("fp32", u, pts, run)
    assert _only(rep, "density") == ["density"] and rep["density"]["worst"] == M


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_09_the_srgb_flag_ignored(prec):
    u, pts, run = _run(prec, "varied", RR.REF_SRGB, fault="nosrgb")
    assert _only(_check(prec, u, pts, run, RR.REF_SRGB), "rgb") == ["rgb"]
    u, pts, run = _run(prec, "varied", RR.REF_SRGB)
    assert _only(_check(prec, u, pts, run, 0), "rgb") == ["rgb"]                    # and the other way round


def test_fault_10_one_flipped_mask_bit():
    u, pts, run = _run("bf16")
    run["masks"][12][41, 77] = ~run["masks"][12][41, 77]
    rep = _check("bf16", u, pts, run)
    assert _only(rep, "mask") == ["mask"] and rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (12, 41, 77)
    with pytest.raises(AssertionError, match="mask"):
        RR.assert_forward("flipped mask bit", rep)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_11_a_missing_1e_7_for_a_tiny_normal(prec):
    """the varied set: a sample whose normal unit is switched off has |n| = |bias| = 3.7e-7"""
    u, pts, run = _run(prec, "varied", fault="no1e-7")
    tiny = run["aux"][:, 0:3].norm(dim=1) < 1e-6
    assert 8 < int(tiny.sum()) < M - 8
    rep = _check(prec, u, pts, run)
    bad = _only(rep, "normal")
    assert bool(tiny[rep["normal"]["where"][0]]) and set(bad) <= {"normal", "ide", "ndot"}


def test_a_perturbed_spec_value_and_a_nonzero_aux_padding_are_caught():
    u, pts, run = _run("fp32")
    run["aux"][17, 15] = 1e-30
    run["aux"][3, 12] += 2.0 ** -10
    rep = _check("fp32", u, pts, run)
    bad = RR.failing(rep)
    assert "auxpad" in bad and "spec" in bad and rep["spec"]["where"] == (3, 1) and "rgb" in bad
