"""The yardstick of tests/test_gpu_forward_layers.py, tested on the CPU (tests/forward_ref.py): an honest emulation of the forward kernels
-- torch fp32 matmul, bias added in, round-to-nearest bf16 cast, rows placed into slot order -- must sit inside every bound, and each of
seven planted faults must be reported by the same comparators; the unpacker's index map must be a bijection for all four layouts and
must invert a Python packer written from the same header."""
import pytest
import torch

import backward_ref as R
import forward_ref as F
import torch_spec as T
import weights as W

M = 64


def _state(name, tag):
    hidden = 128 if name.endswith("128") else 256
    sd = W.proposal_state(tag, hidden=hidden) if name.startswith("prop") else W.mip_state(tag, hidden=hidden)
    return [v for k, v in sd.items() if k.endswith(".weight")], [v for k, v in sd.items() if k.endswith(".bias")]


def _blob(name, prec, tag):
    lay = F.LAYOUTS[name]
    ws, bs = _state(name, tag)
    fw = fb = None
    if lay.fold:
        fw, fb = ws[9][:, :256] @ ws[7], ws[9][:, :256] @ bs[7] + bs[9]                  # fp32, in whatever order torch adds
    mats, biases = F.layer_masters(lay, ws, bs, fw, fb)
    return lay, ws, bs, mats, biases, fw, fb, F.pack(lay, prec, mats, biases, fw, fb)


def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _inputs(net, prec):
    gen = torch.Generator().manual_seed(11)
    x = torch.rand(M, 3, generator=gen) * 2 - 1
    ex = R.element(torch.cat((x, T._pe(x, 10)), -1), prec)
    if net == "prop":
        return R.reference_to_slot(ex, 10, 4), ex, None
    d = torch.randn(M, 3, generator=gen)
    d = d / d.norm(dim=-1, keepdim=True)
    ed = R.element(torch.cat((d, T._pe(d, 4)), -1), prec)
    return torch.cat((R.reference_to_slot(ex, 10, 4), R.reference_to_slot(ed, 4, 2)), -1), ex, ed


def _emulate(net, prec, u, ex, ed, fault=None, at=None, pick=None):
    """the kernels' arithmetic, honestly: fp32 products and sums in torch's order, bias added in, one round-to-nearest conversion.
    fault / at = a planted fault and the stage it is planted in; pick(x, w, b) -> (j, k) chooses the element it hits."""
    cast = (lambda v: R.element(v, prec)) if fault != "trunc" else _trunc_bf16
    acts, out = {}, torch.zeros(M, 1 if net == "prop" else 4)
    for name, l, kind, ins, dst in F.STAGES[net]:
        x = torch.cat([ex if i == "enc" else (ed if i == "dir" else acts[i]) for i in ins], dim=1).float()
        w, b = u.w[l].float(), u.b[l].float()
        if name == at:
            if fault == "bias":
                j, _ = pick(x, w, b)
                b = b.clone()
                b[j] = 0.0
            elif fault == "kgswap":                                                       # K groups 2 and 5 of the hidden input
                x = x.clone()
                o = x.shape[1] - 256
                x[:, o + 32: o + 48], x[:, o + 80: o + 96] = x[:, o + 80: o + 96].clone(), x[:, o + 32: o + 48].clone()
            elif fault == "skip":                                                         # hidden state where the encoding belongs
                x = torch.cat((acts[3].float()[:, :63], acts[3].float()), dim=1)
            elif fault == "sign":
                j, k = pick(x, w, b)
                w = w.clone()
                w[j, k] = -w[j, k]
        z = x @ w.t() + b
        if kind == "hidden":
            acts[dst] = cast(torch.relu(z))
        elif kind == "linear":
            out[:, dst] = z
        else:
            out[:, dst] = 1.0 / (1.0 + torch.exp(-z))
    return acts, (out[:, 0] if net == "prop" else out)


def _pick_live(x, w, b):
    """an element whose fault shows: the most active input feature k, and the output row j with the largest weight on it among
    the rows that are switched on for at least a quarter of the samples"""
    k = int(x.mean(0).argmax())
    on = (torch.relu(x @ w.t() + b) > 0).float().mean(0) >= 0.25
    j = int((w[:, k].abs() * on).argmax())
    return j, k


def _pick_bias(x, w, b):
    on = (torch.relu(x @ w.t() + b) > 0).float().mean(0) >= 0.25
    return int((b.abs() * on).argmax()), 0


def _run(net, prec, tag, **fault):
    lay, _, _, _, _, _, _, blob = _blob(net, prec, tag)
    u = F.unpack(blob, lay, prec)
    enc, ex, ed = _inputs(net, prec)
    acts, out = _emulate(net, prec, u, ex, ed, **fault)
    return lay, u, acts, enc, out


def _ratios(net, prec, lay, u, acts, enc, out, masks=None):
    return F.ratios(F.check_forward(net, prec, lay, u, acts, enc, out, masks))


@pytest.mark.parametrize("tag", ["small", "he"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["prop", "mip"])
def test_honest_emulation_is_inside_every_bound(net, prec, tag):
    lay, u, acts, enc, out = _run(net, prec, tag)
    masks = {L: a > 0 for L, a in acts.items()}
    rep = F.check_forward(net, prec, lay, u, acts, enc, out, masks)
    F.assert_forward("honest %s %s %s" % (net, prec, tag), rep)
    r = F.ratios(rep)
    assert set(r) == {s[0] for s in F.STAGES[net]} | {"mask"} and all(v <= 1.0 for k, v in r.items() if k != "mask") and r["mask"] == 0
    if prec == "bf16":
        assert max(r["h1"], r["h2"], r["h3"]) > 0.5                                      # round-to-nearest attains its term: no slack to hide in


@pytest.mark.parametrize("net", ["prop", "mip"])
def test_a_truncating_bf16_conversion_is_caught(net):
    r = _ratios(net, "bf16", *_run(net, "bf16", "he", fault="trunc"))
    assert all(r[s] > 1.0 for s in ("h0", "h1", "h2", "h3")), r


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["prop", "mip"])
def test_a_dropped_bias_column_is_caught(net, prec):
    for tag in ("small", "he"):
        r = _ratios(net, prec, *_run(net, prec, tag, fault="bias", at="h1", pick=_pick_bias))
        assert r["h1"] > 1.0 and r["h0"] <= 1.0 and r["h2"] <= 1.0, (tag, r)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["prop", "mip"])
def test_two_swapped_k_groups_are_caught(net, prec):
    for at in ("h2",) if net == "prop" else ("h2", "h4", "h7"):
        r = _ratios(net, prec, *_run(net, prec, "he", fault="kgswap", at=at))
        assert r[at] > 1.0 and all(v <= 1.0 for k, v in r.items() if k != at), (at, r)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_skip_layer_fed_the_hidden_state_is_caught(prec):
    for tag in ("small", "he"):
        r = _ratios("mip", prec, *_run("mip", prec, tag, fault="skip", at="h4"))
        assert r["h4"] > 1.0 and all(v <= 1.0 for k, v in r.items() if k != "h4"), (tag, r)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["prop", "mip"])
def test_one_flipped_weight_sign_is_caught(net, prec):
    for tag in ("small", "he"):
        for at in ("h0", "h3") if net == "prop" else ("h0", "h4", "h7"):
            r = _ratios(net, prec, *_run(net, prec, tag, fault="sign", at=at, pick=_pick_live))
            assert r[at] > 1.0 and all(v <= 1.0 for k, v in r.items() if k != at), (tag, at, r)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("net", ["prop", "mip"])
def test_a_row_duplicated_into_its_neighbour_is_caught(net, prec):
    lay, u, acts, enc, out = _run(net, prec, "he")
    acts[2] = acts[2].clone()
    acts[2][38] = acts[2][37]
    rep = F.check_forward(net, prec, lay, u, acts, enc, out)
    r = F.ratios(rep)
    assert r["h2"] > 1.0 and rep["h2"]["where"][0] == 38 and r["h3"] > 1.0 and rep["h3"]["where"][0] == 38, rep
    assert all(v <= 1.0 for k, v in r.items() if k not in ("h2", "h3")), r
    with pytest.raises(AssertionError, match="h2"):
        F.assert_forward("duplicated row", rep)


@pytest.mark.parametrize("net", ["prop", "mip"])
def test_one_flipped_mask_bit_is_caught(net):
    lay, u, acts, enc, out = _run(net, "bf16", "he")
    masks = {L: a > 0 for L, a in acts.items()}
    masks[1][41, 77] = ~masks[1][41, 77]
    rep = F.check_forward(net, "bf16", lay, u, acts, enc, out, masks)
    assert rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (1, 41, 77)
    with pytest.raises(AssertionError, match="mask"):
        F.assert_forward("flipped mask bit", rep)


def test_mask_rows_reads_the_records_backward_ref_describes():
    gen = torch.Generator().manual_seed(5)
    for width in (256, 128):
        want = torch.rand(96, width, generator=gen) < 0.3
        block = torch.zeros(3 * 1024, dtype=torch.uint8)
        for m, f in torch.nonzero(want).tolist():
            byte, bit = R.mask_bit(m, f)
            block[byte] |= 1 << bit
        assert torch.equal(F.mask_rows(block, width), want)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip", "prop128", "mip128"])
def test_the_index_map_is_a_bijection(name, prec):
    lay = F.LAYOUTS[name]
    assert F.map_is_bijection(lay, prec)
    assert all(lay.START[l] + lay.NKG[l] * lay.NFB[l] == (lay.START[l + 1] if l + 1 < lay.N_LAYERS else lay.USED_FRAGS) for l in range(lay.N_LAYERS))
    assert all(lay.BIAS_OFF[l] + 32 * lay.NFB[l] == (lay.BIAS_OFF[l + 1] if l + 1 < lay.N_LAYERS else lay.N_BIAS) for l in range(lay.N_LAYERS))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip", "prop128", "mip128"])
def test_the_unpacker_inverts_the_python_packer(name, prec):
    lay, ws, bs, mats, biases, fw, fb, blob = _blob(name, prec, "he")
    u = F.unpack(blob, lay, prec)
    for l in range(lay.N_LAYERS):
        assert torch.equal(u.w[l].double(), R.operand(mats[l], prec)), (name, prec, l)
        assert u.pad[l].numel() == 512 * lay.NKG[l] * lay.NFB[l] - lay.rows[l] * lay.in_f[l] and not bool((u.pad[l] != 0).any())
        assert torch.equal(u.b[l], biases[l]) and not bool((u.bpad[l] != 0).any())
    assert u.tail.numel() == (lay.N_FRAGS - lay.USED_FRAGS) * 512 and not bool((u.tail != 0).any())
    if lay.fold:
        assert torch.equal(u.fold_w, fw) and torch.equal(u.fold_b, fb)
    # a slip that the round trip alone could hide (packer and unpacker share slot_column): the skip layer's K order, spelled out
    if name == "mip":
        pos, row, col = F.index_map(lay, 4, prec)
        first = col[:512]                                                                # fragment (fb 0, kg 0): encoding K group 0
        assert int(first.max()) < 63 and int(col[2 * 4 * 512: 2 * 4 * 512 + 512].min()) >= 63      # ... K group 4 = hidden features 0..15
