"""The yardstick of tests/test_gpu_backward_layers.py, tested on the CPU: the stage formulas of tests/backward_ref.py chained end to end
in fp64 on a torch forward of torch_spec.proposal_expr / mip_expr must reproduce torch.autograd (layer table, skip-layer column split,
fold / un-fold algebra, slot-to-column permutation), and its bounds must hold for an fp32 emulation of the accumulation alone while
still catching a zeroed element or one dropped probe."""
import torch
import torch.nn.functional as F

import backward_ref as R
import torch_spec as T
import weights as W


def _params(state):
    ws = [v.double() for k, v in state.items() if k.endswith(".weight")]
    bs = [v.double() for k, v in state.items() if k.endswith(".bias")]
    return ws, bs


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_proposal_stage_formulas_equal_autograd():
    for tag in ("small", "he"):
        ws, bs = _params(W.proposal_state(tag))
        gen = torch.Generator().manual_seed(3)
        M = 300
        pts = torch.rand(M, 3, generator=gen, dtype=torch.float64) * 2 - 1
        g = torch.randn(M, generator=gen, dtype=torch.float64)
        enc = torch.cat((pts, T._pe(pts, 10)), -1)
        acts, h = {}, enc
        for i in range(4):
            h = acts[i] = T.lin_relu(h, ws[i], bs[i])
        assert torch.equal(T.lin(h, ws[4], bs[4]).squeeze(-1), T.proposal_expr(pts, ws, bs))
        head = torch.zeros(M, 16, dtype=torch.float64)
        head[:, 0] = g
        deltas = {}
        for L in R.PROP_ORDER:
            d_in, w = R.prop_stage(L, head, deltas, ws)
            deltas[L] = (d_in @ w) * (acts[L] > 0)
        enc_ref, pad = R.slot_to_reference(R.reference_to_slot(enc, 10, 4), 10)           # through the slot order and back
        assert torch.equal(enc_ref, enc) and pad.shape[1] == 1
        refs = R.prop_grad_refs(head, deltas, acts, enc_ref, 8, "fp32")
        leaves = [t.clone().requires_grad_(True) for t in ws + bs]
        want = torch.autograd.grad(T.proposal_expr(pts, leaves[:5], leaves[5:]), leaves, g)
        for i in range(5):
            assert _rel(refs["w%d" % i][0].reshape(want[i].shape), want[i]) <= 1e-10, (tag, "w", i)
            assert _rel(refs["b%d" % i][0].reshape(want[5 + i].shape), want[5 + i]) <= 1e-10, (tag, "b", i)


def test_mip_stage_formulas_equal_autograd():
    for tag in ("small", "he"):
        ws, bs = _params(W.mip_state(tag))
        gen = torch.Generator().manual_seed(4)
        M = 300
        pts = torch.cat((torch.rand(M, 3, generator=gen, dtype=torch.float64) * 2 - 1, torch.randn(M, 3, generator=gen, dtype=torch.float64)), -1)
        g4 = torch.randn(M, 4, generator=gen, dtype=torch.float64)
        x, d = pts[:, :3], pts[:, 3:] / pts[:, 3:].norm(dim=-1, keepdim=True)
        ex, ed = torch.cat((x, T._pe(x, 10)), -1), torch.cat((d, T._pe(d, 4)), -1)
        acts, h = {}, ex
        for i in range(4):
            h = acts[i] = T.lin_relu(h, ws[i], bs[i])
        h = torch.cat((ex, h), -1)
        for i in range(4, 7):
            h = acts[i] = T.lin_relu(h, ws[i], bs[i])
        w_fold = ws[9][:, :256] @ ws[7]
        acts[7] = F.relu(h @ w_fold.t() + ed @ ws[9][:, 256:].t() + (ws[9][:, :256] @ bs[7] + bs[9]))      # the folded form of the forward
        rgbo = torch.cat((torch.sigmoid(T.lin(acts[7], ws[10], bs[10])), T.lin(h, ws[8], bs[8])), -1)
        assert _rel(rgbo, T.mip_expr(pts, ws, bs)) <= 1e-12
        head = torch.zeros(M, 16, dtype=torch.float64)
        o = rgbo[:, :3]
        head[:, :3] = (g4[:, :3] * (1.0 - o)) * o
        head[:, 3] = g4[:, 3]
        deltas = {}
        for L in R.MIP_ORDER:
            d_in, w = R.mip_stage(L, head, deltas, ws, w_fold)
            deltas[L] = (d_in @ w) * (acts[L] > 0)
        slot = torch.cat((R.reference_to_slot(ex, 10, 4), R.reference_to_slot(ed, 4, 2)), -1)                # slot 8: K groups 0..3 | 4..5
        ex_ref, _ = R.slot_to_reference(slot[:, :64], 10)
        ed_ref, _ = R.slot_to_reference(slot[:, 64:], 4)
        assert torch.equal(ex_ref, ex) and torch.equal(ed_ref, ed)
        refs = R.mip_grad_refs(head, deltas, acts, ex_ref, ed_ref, ws, bs, 8, "fp32")
        leaves = [t.clone().requires_grad_(True) for t in ws + bs]
        want = torch.autograd.grad(T.mip_expr(pts, leaves[:11], leaves[11:]), leaves, g4)
        assert sorted(refs) == sorted(["w%d" % i for i in range(11)] + ["b%d" % i for i in range(11)])
        for i in range(11):
            assert _rel(refs["w%d" % i][0].reshape(want[i].shape), want[i]) <= 1e-10, (tag, "w", i)
            assert _rel(refs["b%d" % i][0].reshape(want[11 + i].shape), want[11 + i]) <= 1e-10, (tag, "b", i)


def _bf16(t):
    return t.to(torch.bfloat16).float()


def test_chain_bound_holds_for_fp32_accumulation_and_bites():
    """bf16 operands, K = 256: exact products added sequentially in fp32 in a few random orders, one RNE to bf16 -- inside the bound;
    a chain element set to zero is outside it almost everywhere.  fp32 mode: rounded products, the same orders."""
    gen = torch.Generator().manual_seed(7)
    M, K, N = 96, 256, 256
    d = _bf16(torch.randn(M, K, generator=gen) * torch.rand(M, 1, generator=gen))
    w = _bf16(torch.randn(K, N, generator=gen) * 0.09)
    act = torch.ones(M, N)
    worst = {"bf16": 0.0, "fp32": 0.0}
    for trial in range(3):
        order = torch.randperm(K, generator=gen)
        acc = torch.zeros(M, N)
        for k in order.tolist():
            acc = acc + d[:, k: k + 1] * w[k: k + 1, :]                     # (bf16 x bf16 is exact in fp32; every addition rounds to fp32)
        for prec, got in (("bf16", acc.to(torch.bfloat16)), ("fp32", acc)):
            rep = R.check_chain_layer(got, d, w, act, prec)
            R.assert_chain_layer("emulated %s layer" % prec, rep)
            worst[prec] = max(worst[prec], rep["worst"])
    assert worst["bf16"] > 0.5                                               # round-to-nearest attains its term: no slack to hide in
    s, a = R.contract(d, w)
    for prec in ("bf16", "fp32"):
        caught = (s.abs() > R.chain_tol(s, a, K, prec)).double().mean().item()
        assert caught >= 0.99, (prec, caught)
    trunc = (acc.view(torch.int32) & -65536).view(torch.float32)           # a truncating fp32 -> bf16 conversion does not fit
    assert R.check_chain_layer(trunc.to(torch.bfloat16), d, w, act, "bf16")["worst"] > 1.0
    rep = R.check_chain_layer(acc.to(torch.bfloat16), d, w, torch.zeros(M, N), "bf16")      # delta where the unit was off
    assert rep["off_nonzero"] > 0
    try:
        R.assert_chain_layer("masked", rep)
    except AssertionError:
        pass
    else:
        raise AssertionError("a delta on a switched-off unit was accepted")


def test_wgrad_bound_holds_for_blocked_partial_sums_and_bites():
    """512-probe comb: bf16 delta x bf16 activations, blocked fp32 partial sums ("workgroups") combined in fp32 -- far inside the bound; one
    dropped probe is outside it on (nearly) every element it touches; 32 of 70 001 dense samples dropped are NOT seen (why the comb exists)."""
    gen = torch.Generator().manual_seed(9)
    n, No, Ni, n_wg = 512, 64, 128, 37
    d = _bf16(torch.randn(n, No, generator=gen))                            # (plain random operands: every probe carries the same weight)
    x = _bf16(torch.relu(torch.randn(n, Ni, generator=gen)))
    head = torch.ones(n, 1)

    def blocked(dd, xx):
        parts = []
        for blk in torch.tensor_split(torch.arange(dd.shape[0]), n_wg):
            acc = torch.zeros(No, Ni)
            for m in blk.tolist():
                acc = acc + dd[m][:, None] * xx[m][None, :]
            parts.append(acc)
        tot = torch.zeros(No, Ni)
        for p in parts:
            tot = tot + p
        return tot
    s, a = R.outer(d, x)
    tol = R.wgrad_tol(a, int((head != 0).sum()), n_wg, "bf16")
    got = blocked(d, x)
    assert float(((got.double() - s).abs() / tol).max()) <= 1.0
    sb, ab = R.outer(d, None)
    assert float(((d.sum(0).double() - sb).abs() / R.wgrad_tol(ab, n, n_wg, "bf16")).max()) <= 1.0
    for drop in (0, 200, 511):
        keep = torch.arange(n) != drop
        miss = blocked(d[keep], x[keep])
        touched = (d[drop][:, None] * x[drop][None, :]) != 0
        caught = (((miss.double() - s).abs() > tol) & touched).sum().item() / touched.sum().item()
        assert caught >= 0.90, (drop, caught)
    rep = R.grad_ratios({"w1": (s, tol)}, {"w1": miss})
    try:
        R.assert_grads("one probe dropped", rep)
    except AssertionError as e:
        assert "w1" in str(e)
    else:
        raise AssertionError("a dropped probe was accepted")
    # dense: the worst-case bound of 70 001 samples is wider than one subtile's share
    Md = 70001
    dd = _bf16(torch.randn(Md, 8, generator=gen))
    xd = _bf16(torch.relu(torch.randn(Md, 8, generator=gen)))
    sd, ad = R.outer(dd, xd)
    told = R.wgrad_tol(ad, Md, n_wg, "bf16")
    sm, _ = R.outer(dd[32:], xd[32:])
    assert not bool(((sm - sd).abs() > told).any())


def test_comb_runs_cover_every_subtile_and_boundary():
    for tile in (128, 256):
        for M in (1, 31, 33, 255, 256, 257, 1000, 70001):
            runs = R.comb_runs(M, tile)
            hit = set()
            for r in runs:
                assert len(r) <= 512 and len({m // 32 for m in r}) == len(r) and all(0 <= m < M for m in r)
                hit.update(r)
            assert {m // 32 for m in hit} == set(range((M + 31) // 32))
            need = {0, M - 1} | {t for t in range(tile, M, tile)} | {t - 1 for t in range(tile, M + 1, tile)}
            assert need <= hit, (tile, M, sorted(need - hit))
            assert len({m % 32 for m in hit}) > 1 or M == 1
