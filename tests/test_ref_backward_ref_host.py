"""The yardstick of tests/test_gpu_ref_backward_layers.py, tested on the CPU (tests/ref_backward_ref.py): the stage formulas a-f chained
end to end in fp64 on a torch fp64 Ref-NeRF forward reproduce torch.autograd's parameter gradients and RefNeRF.get_grad (with and
without sRGB, with and without the scene contraction); an honest fp32 / bf16 emulation of the backward sits inside every bound; each of
nine planted faults is reported by the stage it belongs to.  A fault is planted in the emulated data, never in repository code."""
import pytest
import torch
import torch.nn.functional as Fn

import backward_ref as R
import ref_backward_ref as RB
import ref_forward_ref as RR
import torch_spec as T
import weights as W
from nerf_amd.ref_func import ide_table
from oracle import nerf_oracle as O
from test_ref_forward_ref_host import _noise, _operands, _state, inputs

M = 64
TABLE = ide_table(4)
NAMES = (["spa_block1.%d" % i for i in (0, 2, 4, 6)] + ["spa_block2.%d" % i for i in (0, 2, 4, 6)] +
         ["bottle_neck", "norm_col_tint_head", "rho_tau_head"] + ["dir_block1.%d" % i for i in (0, 2, 4, 6)] +
         ["dir_block2.%d" % i for i in (0, 2, 4, 6)] + ["spec_rgb_head.0"])          # ops.ref_backward's tensor order


def _g_out(n, seed=5):
    return torch.randn(n, 7, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ composition == autograd (fp64)
def forward64(P, x, d, noise, flags):
    """RefNeRF.forward in fp64 with every intermediate the backward's stages read -> (out7, run pieces)"""
    lin = lambda name, t: Fn.linear(t, P[name + ".weight"], P[name + ".bias"])
    ex = torch.cat((x, T._pe(x, 10)), -1)
    acts, h = {}, ex
    for j, i in enumerate((0, 2, 4, 6)):
        h = acts[j] = Fn.relu(lin("spa_block1.%d" % i, h))
    h = torch.cat((ex, h), -1)
    for j, i in enumerate((0, 2, 4, 6)):
        h = acts[4 + j] = Fn.relu(lin("spa_block2.%d" % i, h))
    nct, rt = lin("norm_col_tint_head", h), lin("rho_tau_head", h)
    bn = lin("bottle_neck", h) + (0 if noise is None else noise)
    n0 = nct[:, 0:3]
    normal = -n0 / (n0.norm(dim=-1, keepdim=True) + RR.C_1E7)
    dot = (d * normal).sum(-1, keepdim=True)
    refl = d - 2.0 * dot * normal
    ide = O.ide_encode(refl, Fn.softplus(rt[:, 0:1] - 1.0), 4)
    allin = torch.cat((bn, ide, dot), -1)
    r = allin
    for j, i in enumerate((0, 2, 4, 6)):
        r = acts[9 + j] = Fn.relu(lin("dir_block1.%d" % i, r))
    r = torch.cat((allin, r), -1)
    for j, i in enumerate((0, 2, 4, 6)):
        r = acts[13 + j] = Fn.relu(lin("dir_block2.%d" % i, r))
    spec = lin("spec_rgb_head.0", r)
    if flags & RR.REF_SRGB:
        x_lin = torch.sigmoid(spec) * torch.sigmoid(nct[:, 6:9]) + torch.sigmoid(nct[:, 3:6] - RR.C_LOG3)
        s1 = (211.0 * torch.maximum(torch.full_like(x_lin, RR.C_EPS), x_lin) ** RR.C_P - 11.0) / 200.0
        rgb = torch.where(x_lin <= RR.C_KNEE, RR.C_1292 * x_lin, s1)
    else:
        rgb = torch.sigmoid(spec) * torch.sigmoid(nct[:, 6:9]) + torch.sigmoid(nct[:, 3:6])
    aux = torch.cat((nct[:, 0:3], rt[:, 0:1], nct[:, 3:6], rt[:, 1:2], nct[:, 6:9], spec, torch.zeros_like(spec[:, :2])), -1)
    return torch.cat((rgb, rt[:, 1:2], normal), -1), {"acts": acts, "aux": aux, "s8": RR.join_slot8(bn, torch.cat((ide, dot), -1), ex)}


def _compose(ws, fwd, d, g_out, flags):
    """stages a-e chained in fp64: every stage's reference VALUE feeds the next"""
    w = [t.double() for t in ws[:19]]
    acts, aux = fwd["acts"], fwd["aux"]
    n = aux.shape[0]
    masks = {L: acts[L] > 0 for L in RR.HIDDEN_SLOTS}
    s8d = torch.zeros(n, RB.S8D_WIDTH, dtype=torch.float64)
    s8d[:, 144:147] = RB.spec_head_ref(g_out, aux, flags)[0]
    deltas = {}
    for L in RB.DIR_SLOTS:
        d_in, wm = RB.dir_stage(L, s8d[:, 144:147], deltas, w)
        deltas[L] = (d_in @ wm) * masks[L]
    da = torch.zeros(n, 192, dtype=torch.float64)
    da[:, :167] = deltas[13] @ w[14][:, :167] + deltas[9] @ w[10]
    s8d[:, 128:139] = RB.heads_delta_ref(g_out, aux, d, da, TABLE, flags)[0]
    s8d[:, :128] = da[:, :128]
    for L in RB.SPA_SLOTS:
        d_in, wm = RB.spa_stage(L, s8d, deltas, w)
        deltas[L] = (d_in @ wm) * masks[L]
    run = {"deltas": deltas, "s8d": s8d, "acts": acts, "s8": fwd["s8"]}
    return {k: v[0] for k, v in RB.grad_refs("fp32", run, 1).items()}, masks


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("flags", [0, RR.REF_SRGB])
@pytest.mark.parametrize("tag", ["he", "varied"])
def test_stages_compose_to_autograd_and_get_grad(tag, flags, contract):
    sd = {k: v.double() for k, v in _state(tag).items()}
    ws, _ = RR.kernel_tensors(_state(tag), TABLE)
    ws = [t.double() for t in ws]
    n = 96
    pts = inputs(n, 21, wide=contract).double()
    g_out, noise = _g_out(n).double(), _noise(n).double()
    x = pts[:, :3].clone().requires_grad_(True)
    pos = O.contract(x) if contract else x
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out7, fwd = forward64(P, pos, pts[:, 3:6], noise, flags)
    want = O.ref_forward({k: v for k, v in sd.items()}, torch.cat((pos, pts[:, 3:6]), -1)[None].detach(), noise=noise[None], use_srgb=bool(flags))
    assert float((out7[:, :4].detach() - want[0][0]).abs().max()) < 1e-6 and float((out7[:, 4:].detach() - want[1][0]).abs().max()) < 1e-6
    keys = [k + s for k in NAMES for s in (".weight", ".bias")]
    grads = torch.autograd.grad((out7 * g_out).sum(), [P[k] for k in keys], retain_graph=True)
    fwd = {"acts": {k: v.detach() for k, v in fwd["acts"].items()}, "aux": fwd["aux"].detach(), "s8": fwd["s8"].detach()}
    got, masks = _compose(ws, fwd, pts[:, 3:6], g_out, flags)
    lim = 1e-6 if flags else 1e-9            # (sRGB: the kernels' fp32 constants 12.92, 5/12, log 3 against autograd of the same expression)
    for i in range(20):
        assert _rel(got["w%d" % i].reshape(grads[2 * i].shape), grads[2 * i]) <= lim, (tag, flags, "w", i)
        assert _rel(got["b%d" % i].reshape(grads[2 * i + 1].shape), grads[2 * i + 1]) <= lim, (tag, flags, "b", i)
    # stage f: d density / d position and RefNeRF.get_grad
    scale = torch.rand(n, generator=torch.Generator().manual_seed(2), dtype=torch.float64) + 0.5
    denc, _ = RB.denc_ref("ref", "fp32", ws, {L: masks[L] for L in range(8)})
    grad, _ = RB.pe_grad_ref(Fn.pad(denc, (0, 1)), x.detach(), scale, contract)
    auto, = torch.autograd.grad(out7[:, 3], x, torch.ones(n, dtype=torch.float64), retain_graph=True)
    assert _rel(grad, auto * scale[:, None]) <= 1e-9
    unscaled, _ = RB.pe_grad_ref(Fn.pad(denc, (0, 1)), x.detach(), None, contract)
    nrm = unscaled.norm(dim=-1, keepdim=True)
    assert _rel(unscaled / torch.maximum(torch.full_like(nrm, 1e-5), nrm), O.get_grad(out7[:, 3], x)) <= 1e-9


def test_proposal_density_chain_composes_to_autograd():
    state = W.proposal_state("he")
    ws = [v.double() for k, v in state.items() if k.endswith(".weight")]
    bs = [v.double() for k, v in state.items() if k.endswith(".bias")]
    for contract in (False, True):
        x = inputs(96, 4, wide=contract)[:, :3].double().requires_grad_(True)
        pos = O.contract(x) if contract else x
        h, masks = torch.cat((pos, T._pe(pos, 10)), -1), {}
        for i in range(4):
            h = T.lin_relu(h, ws[i], bs[i])
            masks[i] = h.detach() > 0
        dens = T.lin(h, ws[4], bs[4]).squeeze(-1)
        denc, _ = RB.denc_ref("prop", "fp32", ws, masks)
        grad, _ = RB.pe_grad_ref(Fn.pad(denc, (0, 1)), x.detach(), None, contract)
        auto, = torch.autograd.grad(dens.sum(), x)
        assert _rel(grad, auto) <= 1e-9


# ------------------------------------------------------------------------------------------------ the honest emulation
def _run(prec, tag="he", flags=0, noise=None, contract=False, fault=None, comb=False):
    u = _operands(tag, prec)[2]
    ws, _ = RR.kernel_tensors(_state(tag), TABLE)
    pts = inputs(M, 11, wide=contract)
    fwd = RR.emulate(prec, u, pts, noise, flags, contract)
    g = _g_out(M)
    if comb:
        keep = torch.zeros(M, 1)
        keep[[3, 40]] = 1.0
        g = g * keep
    return ws, pts, fwd, RB.emulate(prec, ws, fwd, pts[:, 3:6], g, TABLE, flags, fault)


def _check(prec, ws, run, flags=0, rows=None, grads=None):
    rep = RB.check_elementwise(prec, run, TABLE, flags)
    rep.update(RB.check_chains(prec, RB.operands(ws, prec), run))
    g = R.grad_ratios(RB.grad_refs(prec, run, 4, rows), run["grads"] if grads is None else grads)
    return rep, g


ALL = {"spec-head", "spec-zero", "heads-delta", "heads-zero", "bn-order", "dallin", "dallin-pad", "off-nonzero"} | \
      {"D%d" % L for L in RB.DIR_SLOTS} | {"S%d" % L for L in RB.SPA_SLOTS}


@pytest.mark.parametrize("flags", [0, RR.REF_SRGB])
@pytest.mark.parametrize("tag", ["small", "he", "varied"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_honest_emulation_is_inside_every_bound(prec, tag, flags):
    for noise in (None, _noise(M)):
        ws, pts, fwd, run = _run(prec, tag, flags, noise)
        rep, g = _check(prec, ws, run, flags)
        RB.assert_report("honest %s %s flags %d" % (prec, tag, flags), rep)
        assert set(rep) == ALL and len(g) == 40
        R.assert_grads("honest products", g)
        if prec == "bf16" and tag != "small":
            r = RB.ratios(rep)
            assert max(r["D12"], r["S3"], r["dallin"]) > 0.3                 # round-to-nearest attains its term: no slack to hide in


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("net", ["ref", "prop"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_honest_density_gradient_is_inside_its_bounds(prec, net, contract):
    rep, _ = _density(prec, net, contract)
    RB.assert_report("honest density gradient %s %s" % (prec, net), rep)


def _density(prec, net, contract, fault=None, flip=None):
    """flip = (slot, sample, index among the set bits): a mask bit cleared for the density chain alone"""
    pts = inputs(M, 11, wide=contract)
    scale = torch.rand(M, generator=torch.Generator().manual_seed(3)) + 0.5
    unit = torch.zeros(M, 7)
    unit[:, 3] = 1.0
    if net == "ref":
        ws, _ = RR.kernel_tensors(_state("he"), TABLE)
        ws = ws[:19]
        fwd = RR.emulate(prec, _operands("he", prec)[2], pts, None, 0, contract)
        masks = fwd["masks"]
        deltas = RB.emulate(prec, ws, fwd, pts[:, 3:6], unit, TABLE)["deltas"]
    else:
        state = W.proposal_state("he")
        ws = [v for k, v in state.items() if k.endswith(".weight")]
        bs = [v for k, v in state.items() if k.endswith(".bias")]
        pos = T.contract_expr(pts[:, :3]) if contract else pts[:, :3]
        h, masks = torch.cat((pos, T._pe(pos, 10)), -1), {}
        for i in range(4):
            h = R.element(T.lin_relu(h.float(), R.operand(ws[i], prec).float(), bs[i]), prec)
            masks[i] = h > 0
        w32 = [R.operand(t, prec).float() for t in ws]
        deltas = {3: R.element(w32[4] * masks[3], prec)}                           # prop_bwd_kernel with g_density = 1
        for L in (2, 1, 0):
            deltas[L] = R.element((deltas[L + 1].float() @ w32[L + 1]) * masks[L], prec)
    used = masks
    if flip is not None:
        slot, m, i = flip
        used = {k: v.clone() for k, v in masks.items()}
        used[slot][m, int(torch.nonzero(used[slot][m])[i])] = False
    d_enc, out = RB.emulate_density(net, prec, ws, used, pts, scale, contract, fault)
    w = [R.operand(t, prec) for t in ws]
    return RB.check_density_grad(net, prec, w, masks, d_enc, pts, scale, contract, out, deltas), (d_enc, out)


# ------------------------------------------------------------------------------------------------ the nine planted faults
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_1_a_sign_flip_in_one_ide_term(prec):
    ws, pts, fwd, run = _run(prec, "varied", fault="ide_sign")
    rep, _ = _check(prec, ws, run)
    assert "heads-delta" in RB.failing(rep) and set(RB.failing(rep)) <= {"heads-delta", "S7"}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_2_the_reflections_factor_two_dropped(prec):
    ws, pts, fwd, run = _run(prec, "he", fault="refl2")
    rep, _ = _check(prec, ws, run)
    assert "heads-delta" in RB.failing(rep) and rep["heads-delta"]["where"][1] in (128, 129, 130)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_3_a_finalize_window_shifted_by_one_column(prec):
    ws, pts, fwd, run = _run(prec)
    for name, col in (("w4", 63), ("w11", 128), ("w15", 167)):
        grads = dict(run["grads"])
        g = grads[name].clone()
        g[:, col - 1: -1] = grads[name][:, col:]                                 # the second window written one column early
        grads[name] = g
        _, rg = _check(prec, ws, run, grads=grads)
        assert [k for k, v in rg.items() if not v <= 1.0] == [name]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_4_two_head_rows_swapped(prec):
    """rows 131 (roughness) and 135 (density) of the head block: rho_tau_head's two rows trade places"""
    ws, pts, fwd, run = _run(prec, "varied")
    grads = dict(run["grads"])
    grads["w10"], grads["b10"] = grads["w10"].flip(0), grads["b10"].flip(0)
    _, rg = _check(prec, ws, run, grads=grads)
    assert sorted(k for k, v in rg.items() if not v <= 1.0) == ["b10", "w10"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_5_a_skip_side_output_in_the_wrong_block(prec):
    ws, pts, fwd, run = _run(prec, fault="skipblock")
    rep, _ = _check(prec, ws, run)
    assert "dallin" in RB.failing(rep) and "dallin-pad" in RB.failing(rep)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_6_one_subtile_dropped_from_one_product(prec):
    ws, pts, fwd, run = _run(prec, comb=True)
    rows = torch.tensor([3, 40])
    _, rg = _check(prec, ws, run, rows=rows)
    R.assert_grads("honest comb", rg)
    grads = dict(run["grads"])
    grads["w12"] = run["deltas"][10][:32].float().t() @ run["acts"][9][:32].float()      # the second subtile (sample 40) lost
    _, rg = _check(prec, ws, run, rows=rows, grads=grads)
    assert [k for k, v in rg.items() if not v <= 1.0] == ["w12"]
    hit = (run["deltas"][10][40].float()[:, None] * run["acts"][9][40].float()[None, :]) != 0
    s, tol = RB.grad_refs(prec, run, 4, rows)["w12"]
    assert float((((grads["w12"].double() - s).abs() > tol) & hit).sum()) >= 0.9 * float(hit.sum())        # ... on most elements it touches


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_7_one_padding_row_leaking(prec):
    """the forward fills the rows m >= M with copies of row M - 1: one of them contracted too"""
    ws, pts, fwd, run = _run(prec)
    grads = dict(run["grads"])
    grads["w2"] = grads["w2"] + run["deltas"][2][M - 1].float()[:, None] * run["acts"][1][M - 1].float()[None, :]
    _, rg = _check(prec, ws, run, grads=grads)
    assert [k for k, v in rg.items() if not v <= 1.0] == ["w2"]


@pytest.mark.parametrize("net", ["ref", "prop"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fault_8_the_jacobians_u_ut_term_dropped(prec, net):
    rep, _ = _density(prec, net, True, fault="uut")
    assert RB.failing(rep) == ["pe-grad"]
    pts = inputs(M, 11, wide=True)
    assert float(pts[rep["pe-grad"]["where"][0], :3].norm()) > 1.0


@pytest.mark.parametrize("net", ["ref", "prop"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_mask_bit_lost_in_the_density_chain_is_caught(prec, net):
    """by the bound from the mask records alone in fp32; in bf16 that bound is as large as the signal (seven unstored layers of 2^-8
    each, worst case) and it is the comparison with the stored slots that bites"""
    for slot in (0, 2, 3):
        for m in (5, 33, 63):
            rep, _ = _density(prec, net, False, flip=(slot, m, 3))
            assert "denc-rows" in RB.failing(rep) and rep["denc-rows"]["where"][0] == m
            assert prec == "bf16" or "denc" in RB.failing(rep)


def test_fault_9_a_bf16_d_allin_read_as_fp32():
    ws, pts, fwd, run = _run("bf16", fault="bf16_as_fp32")
    rep, _ = _check("bf16", ws, run)
    assert "heads-delta" in RB.failing(rep) and "bn-order" not in RB.failing(rep)


def test_a_flipped_mask_bit_and_a_nonzero_padding_row_are_caught():
    ws, pts, fwd, run = _run("bf16")
    m, f = 41, int(run["deltas"][12][41].float().abs().argmax())
    run["masks"] = dict(run["masks"])
    run["masks"][12] = run["masks"][12].clone()
    run["masks"][12][m, f] = False
    rep, _ = _check("bf16", ws, run)
    assert RB.failing(rep) == ["D12", "off-nonzero"] and rep["off-nonzero"]["worst"] == 1.0
    ws, pts, fwd, run = _run("bf16")
    run["s8d"][M + 5, 130] = 1.0
    run["s8d"][M + 7, 150] = 1.0
    rep, _ = _check("bf16", ws, run)
    assert RB.failing(rep) == ["heads-zero", "spec-zero"]
