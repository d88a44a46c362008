"""The MLP training backward (nerf_amd/csrc/bwd_kernels.hip) pinned layer by layer and element by element.

Every stage is checked against ITS OWN INPUTS as the kernels dumped them (tests/backward_ref.py holds the fp64 references and the
derivation of the worst-case bounds; tests/test_backward_ref_host.py pins that helper against torch.autograd on the CPU):

  1. dgrad chains: delta_L == round( delta_{L+1} . W^T ) * [act_L > 0] for every chain layer of both networks, fp32 and bf16, with
     delta_{L+1} and act_L read from the dumps; exactly zero where the activation is zero; the head slot and the encoding slot bit for bit.
  2. every weight- and bias-gradient tensor against the fp64 contraction of the dumped rows, dense and with comb probes (at most 512
     samples carry a gradient, so that the bound is far below one sample's share and a lost / duplicated subtile or anything picked
     up from the padding rows m >= M shows on most elements);
  2b. nothing the products consume is left over from an earlier call (arena storage pre-filled with 0x00 / 0xFF bytes: bit-identical);
  3. fp8 dumps: the delta slots are the rounded bf16 slots, the products contract the decoded operands;
  4. negative controls: one flipped sign, one zeroed subtile, one flipped mask bit must be reported by the same comparators.

max(err / tol) of every (network, precision, dump format, stage or tensor) goes through conftest.gate (limit 1)."""
import ctypes
import gc
import time

import pytest
import torch

import backward_ref as R
import weights as W
from conftest import gate

pytestmark = pytest.mark.gpu

BASE_M = (1, 31, 33, 255, 256, 257, 1000, 70001)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import ops
    from nerf_amd._lib import lib

    class NS:
        pass
    ns = NS()
    ns.pkg, ns.ops, ns.lib = nerf_amd, ops, lib
    n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
    ns.n_cu = int(n_cu.value)
    ns.nets = {}
    yield ns
    nerf_amd.set_train_dumps("bf16")
    nerf_amd.set_precision("fp32")


class Net:
    def __init__(self, A, name, tag):
        self.name, self.tag = name, tag
        self.id = A.ops.NET_PROPOSAL if name == "prop" else A.ops.NET_MIP
        state = W.proposal_state(tag) if name == "prop" else W.mip_state(tag)
        self.ws = [v.cuda().contiguous() for k, v in state.items() if k.endswith(".weight")]
        self.bs = [v.cuda().contiguous() for k, v in state.items() if k.endswith(".bias")]
        self.order = R.PROP_ORDER if name == "prop" else R.MIP_ORDER
        self.width = R.PROP_WIDTH if name == "prop" else R.MIP_WIDTH
        self.head_slot = R.PROP_HEAD_SLOT if name == "prop" else R.MIP_HEAD_SLOT
        self.slots = self.head_slot + 1
        self.blobs = {}

    def packed(self, A, prec):
        P = A.ops.BF16 if prec == "bf16" else A.ops.F32
        if prec not in self.blobs:
            self.blobs[prec] = (A.ops.pack_weights(self.id, P, self.ws, self.bs), A.ops.pack_weights_backward(self.id, P, self.ws))
        return self.blobs[prec]

    def operands(self, A, prec):
        """-> (the eleven / five operand matrices in fp64, W_fold as the chain multiplies it) -- W_fold from where the kernel takes it: the
        fp32 matrix pack_weights_backward leaves behind the fragment stream of the blob"""
        w = [R.operand(t, prec) for t in self.ws]
        if self.name == "prop":
            return w, None
        blob = self.packed(A, prec)[1]
        stream = 848 * (1024 if prec == "bf16" else 2048)                          # MipBwdLayout::stream_bytes
        assert blob.numel() == stream + 128 * 256 * 4
        fold32 = blob[stream:].view(torch.float32).view(128, 256).clone()
        return w, (fold32, R.operand(fold32, prec))


def _net(A, name, tag):
    if (name, tag) not in A.nets:
        A.nets[(name, tag)] = Net(A, name, tag)
    return A.nets[(name, tag)]


def _inputs(name, M, seed):
    gen = torch.Generator().manual_seed(seed)
    if name == "prop":
        return (torch.rand(M, 3, generator=gen) * 2 - 1).cuda(), torch.randn(M, generator=gen).cuda()
    pts = torch.cat((torch.randn(M, 3, generator=gen) * 1.5, torch.randn(M, 3, generator=gen)), -1).cuda()
    return pts, torch.randn(M, 4, generator=gen).cuda()


def _codes(A, prec, fmt):
    P = A.ops.BF16 if prec == "bf16" else A.ops.F32
    return P, (A.ops.BF16_F8 if fmt == "fp8" else P)


def _forward(A, net, prec, fmt, pts):
    _, T = _codes(A, prec, fmt)
    pk = net.packed(A, prec)[0]
    return (A.ops.proposal_forward_train if net.name == "prop" else A.ops.mip_forward_train)(pk, T, pts)


def _chain(A, net, prec, fmt, g, out, dump):
    _, T = _codes(A, prec, fmt)
    bwd = net.packed(A, prec)[1]
    if net.name == "prop":
        return A.ops.proposal_backward_chain(bwd, T, g, dump)
    return A.ops.mip_backward_chain(bwd, T, g, out, dump)


def _products(A, net, prec, fmt, M, dump, delta):
    _, T = _codes(A, prec, fmt)
    if net.name == "prop":
        gw, gb = A.ops.proposal_weight_grads(T, M, dump, delta)
    else:
        gw, gb = A.ops.mip_weight_grads(T, M, dump, delta, net.ws, net.bs)
    return R.named_grads(gw, gb)


def _geometry(prec, M):
    tile = R.TILE[prec]
    n_sub = (M + tile - 1) // tile * (tile // 32)
    return n_sub, n_sub * 16 * (1024 if prec == "bf16" else 2048)          # (subtiles, layer stride in bytes)


def _slot_rows(A, net, prec, fmt, M, dump, slot, width):
    """one slot of either dump as (M, width) rows: fp8 hidden slots decoded here, everything else through nerf_amd_train_dump_to_rows"""
    P, _ = _codes(A, prec, fmt)
    if fmt == "fp8" and slot < net.head_slot:
        n_sub, ls = _geometry(prec, M)
        return R.decode_f8_slot(dump, slot, ls, n_sub, width // 16)[:M]
    return A.ops.train_dump_rows(dump, net.id, P, M, slot, width)


def _read(A, net, prec, fmt, M, dump, delta):
    """-> (acts, deltas, head (M, 16), encoding slot rows)"""
    acts = {L: _slot_rows(A, net, prec, fmt, M, dump, L, net.width[L]) for L in net.order}
    deltas = {L: _slot_rows(A, net, prec, fmt, M, delta, L, net.width[L]) for L in net.order}
    head = _slot_rows(A, net, prec, fmt, M, delta, net.head_slot, 16)
    enc = _slot_rows(A, net, prec, fmt, M, dump, net.head_slot, 64 if net.name == "prop" else 96)
    return acts, deltas, head, enc


def _encodings(net, enc):
    """encoding slot rows -> reference column order ((M, 63), (M, 27) or None); the padding features must be zero"""
    ex, pad = R.slot_to_reference(enc[:, :64], 10)
    assert not bool((pad != 0).any())
    if net.name == "prop":
        return ex, None
    ed, pad = R.slot_to_reference(enc[:, 64:96], 4)
    assert not bool((pad != 0).any())
    return ex, ed


def _head_want(A, net, prec, g, out):
    """the head K group as the chain kernels form it: fp32 expression, stored as a dump element (bf16: round to nearest even)"""
    M = g.shape[0]
    want = torch.zeros((M, 16), dtype=torch.float32, device=g.device)
    if net.name == "prop":
        want[:, 0] = g
    else:
        want[:, :4] = R.mip_head_f32(g, out)
    return R.element(want, prec)


ENC_STATS = {}


def _check_encoding(A, net, prec, pts, enc, worst, what):
    """The encoding slot of the activation dump, permuted to the reference's column order, against ops.encode_rows of the same points.

    FINDING (measured on the MI355X): the two are NOT bit-identical.  The pass-through columns (x y z, d / |d|) are; the sines and cosines
    are not, because the training forward evaluates them with its own range reduction and fdlibm polynomials (device_common.h
    sin_quadrant / sincos_quadrant) while encode_rows_kernel calls the math library's sincosf -- two faithful fp32 evaluations that
    differ in the last bit on some elements (first seen: ProposalNetwork, fp32, M = 1).  The weight-gradient kernels consume the DUMPED
    slot (bwd_prop_weight_grads: A(4); bwd_mip_weight_grads: A(8) and A(8, 4)); encode_rows feeds only the layer-by-layer route of
    networks beyond the compiled shapes.  So the first-layer, skip-layer and direction-column gradients of part 2 are compared with the
    dumped slot, and this check asserts what is true of two faithful evaluations, from their stated accuracy rather than from the
    measurement: each is within 1.5 ulp of a value <= 1, i.e. 1.5 * 2^-24, of the exact sine, so fp32 rows differ by at most 3 * 2^-24;
    bf16 rows take octave 0 from either routine and double the angle L - 1 times (the difference doubles with it: 2^(L-1) * 3 * 2^-24)
    before one rounding to bf16, which can land the two on neighbouring bf16 values: one spacing (2^-8 below 1) more.  That is also what
    pins the slot-to-column permutation (a wrong column is off by O(1)).  The number of differing elements is printed with the gates."""
    P, _ = _codes(A, prec, "bf16")
    ex, ed = _encodings(net, enc)
    pairs = [("pos", 10, ex, A.ops.encode_rows(pts[:, :3], 10, P)[:, :63])]
    if ed is not None:
        pairs.append(("dir", 4, ed, A.ops.encode_rows(pts[:, 3:6], 4, P, normalize=True)[:, :27]))
    for key, L, got, want in pairs:
        assert torch.equal(got[:, :3], want[:, :3]), what + ": pass-through columns of the %s encoding slot" % key
        diff = (got.double() - want.double()).abs()
        limit = 3 * R.U24 if prec == "fp32" else 2.0 ** -8 + 2.0 ** (L - 1) * 3 * R.U24
        worst["enc-" + key] = max(worst.get("enc-" + key, 0.0), float(diff.max()) / limit)
        st = ENC_STATS.setdefault((net.name, prec, key), [0, 0])
        st[0] += int((diff != 0).sum()); st[1] += diff.numel()
        assert float(diff.max()) <= limit, "%s: %s encoding slot differs from encode_rows by %.3g (limit %.3g)" % (what, key, float(diff.max()), limit)


def _check_chain(A, net, prec, M, pts, g, out, acts, deltas, head, enc, worst):
    """part 1 on one run; `worst` collects max(err / tol) per stage.  Raises on the exact assertions (head, encoding, masked zeros)."""
    what = "%s %s %s M=%d" % (net.name, prec, net.tag, M)
    P, _ = _codes(A, prec, "bf16")
    assert torch.equal(head, _head_want(A, net, prec, g, out)), what + ": head slot"
    _check_encoding(A, net, prec, pts, enc, worst, what)
    w, fold = net.operands(A, prec)
    for L in net.order:
        d_in, wmat = R.stage(net.name, L, head, deltas, w, fold[1] if fold else None)
        rep = R.check_chain_layer(deltas[L], d_in, wmat, acts[L], prec)
        worst["d%d" % L] = max(worst.get("d%d" % L, 0.0), rep["worst"])
        R.assert_chain_layer(what + " delta slot %d" % L, rep)


def _check_grads(A, net, prec, acts, deltas, head, enc, grads, worst, what, rows=None):
    ex, ed = _encodings(net, enc)
    n_wg = 2 * A.n_cu                                                       # upper bound of wgrad_workgroups for every product
    if net.name == "prop":
        refs = R.prop_grad_refs(head, deltas, acts, ex, n_wg, prec, rows)
    else:
        refs = R.mip_grad_refs(head, deltas, acts, ex, ed, net.ws, net.bs, n_wg, prec, rows)
    assert sorted(refs) == sorted(grads)
    rep = R.grad_ratios(refs, grads)
    for k, v in rep.items():
        worst[k] = max(worst.get(k, 0.0), v)
    R.assert_grads(what, rep)
    return rep


def _emit(prefix, worst):
    """one gate line per stage / tensor; every line is written before the first failure is raised"""
    failed = []
    for k in sorted(worst, key=lambda s: (s[0], int(s[1:]) if s[1:].isdigit() else -1, s)):
        try:
            gate("%s %s max(err/tol)" % (prefix, k), worst[k], 1.0)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def _straddle_M(A, net, prec):
    """sample counts whose subtile count is below, at, just above and not a multiple of every product's workgroup cap
    (wgrad_workgroups: n_wg = min(n_sub, n_cu * {1, 2} / n_jobs)), from the CU count of the device at hand"""
    caps = (A.n_cu // 3, 2 * A.n_cu) if net.name == "prop" else (A.n_cu // 6, A.n_cu, 2 * A.n_cu)
    spt = R.TILE[prec] // 32
    out = set()
    for c in caps:
        at = (c + spt - 1) // spt * spt
        big = (5 * c // 2 + spt - 1) // spt * spt + spt
        if big % c == 0:
            big += spt
        for n_sub in ((c - 1) // spt * spt, at, at + spt, big):
            if n_sub >= spt:
                out.add(n_sub * 32 - 13)
    return sorted(out)


def _fold_matrix_ratio(A, net, prec):
    """the fp32 W_fold the backward pack leaves in the blob is the fp64 product to within a 256-term fused multiply-add chain"""
    fold32 = net.operands(A, prec)[1][0]
    w9a, wb = net.ws[9][:, :256].double(), net.ws[7].double()
    err = (fold32.double() - w9a @ wb).abs()
    tol = 257 * R.U24 * (w9a.abs() @ wb.abs())
    return float((err / tol).max())


@pytest.mark.parametrize("tag", ["small", "he"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_dense_chain_and_products(A, name, prec, tag):
    """Parts 1 and 2 (dense): every sample carries a random upstream gradient.  M covers the tile edges, 70 001, one count at which
    every workgroup of the persistent chains runs three or four tiles (3 n_cu tile + 77: the mask double buffer and the weight ring carry
    state across tiles) and, for the 'he' weights, the counts that straddle the products' workgroup arithmetic."""
    net = _net(A, name, tag)
    t0 = time.time()
    Ms = list(BASE_M) + [3 * A.n_cu * R.TILE[prec] + 77] + (_straddle_M(A, net, prec) if tag == "he" else [])
    chain, prods = {}, {}
    if name == "mip":
        gate("bwd-layers mip %s %s W_fold vs fp64 max(err/tol)" % (prec, tag), _fold_matrix_ratio(A, net, prec), 1.0)
    for M in Ms:
        pts, g = _inputs(name, M, 1000 + M % 997)
        out, dump = _forward(A, net, prec, "bf16", pts)
        delta = _chain(A, net, prec, "bf16", g, out, dump)
        grads = _products(A, net, prec, "bf16", M, dump, delta)
        acts, deltas, head, enc = _read(A, net, prec, "bf16", M, dump, delta)
        _check_chain(A, net, prec, M, pts, g, out, acts, deltas, head, enc, chain)
        _check_grads(A, net, prec, acts, deltas, head, enc, grads, prods, "%s %s %s dense M=%d" % (name, prec, tag, M))
        del dump, delta
    torch.cuda.synchronize()
    print("dense %s %s %s: %d sample counts up to %d in %.1f s; encoding slot elements that differ from encode_rows: %s" % (
        name, prec, tag, len(Ms), max(Ms), time.time() - t0, {k: "%d of %d" % tuple(v) for k, v in ENC_STATS.items() if k[:2] == (name, prec)}))
    _emit("bwd-layers %s %s bf16-dumps %s chain" % (name, prec, tag), chain)
    _emit("bwd-layers %s %s bf16-dumps %s dense" % (name, prec, tag), prods)


def _comb_case(A, net, prec, fmt, M, worst, max_runs=None):
    """Part 2, comb probes: the upstream gradient is nonzero on at most 512 samples per run, one per 32-sample subtile."""
    pts, g_full = _inputs(net.name, M, 77 + M % 991)
    runs = R.comb_runs(M, R.TILE[prec])
    for r, probes in enumerate(runs if max_runs is None else runs[:max_runs]):
        idx = torch.tensor(probes, device="cuda")
        g = torch.zeros_like(g_full)
        g[idx] = g_full[idx]
        out, dump = _forward(A, net, prec, fmt, pts)
        delta = _chain(A, net, prec, fmt, g, out, dump)
        grads = _products(A, net, prec, fmt, M, dump, delta)
        acts, deltas, head, enc = _read(A, net, prec, fmt, M, dump, delta)
        unprobed = torch.ones(M, dtype=torch.bool, device="cuda")
        unprobed[idx] = False
        for L, d in list(deltas.items()) + [("head", head)]:
            assert not bool((d[unprobed] != 0).any()), "%s %s M=%d run %d: delta slot %s is nonzero on an unprobed sample" % (net.name, prec, M, r, L)
        what = "%s %s %s-dumps %s comb M=%d run %d" % (net.name, prec, fmt, net.tag, M, r)
        _check_grads(A, net, prec, acts, deltas, head, enc, grads, worst, what, rows=idx)
        del dump, delta


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_comb_probes_products(A, name, prec):
    net = _net(A, name, "he")
    worst = {}
    t0 = time.time()
    for M in (1, 33, 257, 1000, 70001):
        _comb_case(A, net, prec, "bf16", M, worst)
    torch.cuda.synchronize()
    print("comb %s %s: %.1f s" % (name, prec, time.time() - t0))
    _emit("bwd-layers %s %s bf16-dumps he comb" % (name, prec), worst)


def test_full_size_bf16_mip_products(A):
    """The bench's training batch, 2^14 rays x 128 samples, bf16 MipNeRF, dense; the fp64 reference runs on the device in chunks."""
    net = _net(A, "mip", "he")
    M = (1 << 14) * 128
    t0 = time.time()
    pts, g = _inputs("mip", M, 5)
    out, dump = _forward(A, net, "bf16", "bf16", pts)
    delta = _chain(A, net, "bf16", "bf16", g, out, dump)
    grads = _products(A, net, "bf16", "bf16", M, dump, delta)
    torch.cuda.synchronize()
    t1 = time.time()
    acts, deltas, head, enc = _read(A, net, "bf16", "bf16", M, dump, delta)
    del dump, delta
    worst = {}
    _check_grads(A, net, "bf16", acts, deltas, head, enc, grads, worst, "mip bf16 full size")
    torch.cuda.synchronize()
    print("full size M=%d: kernels %.1f s, reference and comparison %.1f s" % (M, t1 - t0, time.time() - t1))
    _emit("bwd-layers mip bf16 bf16-dumps he dense-2^21", worst)


# ------------------------------------------------------------------------------------------------ 2b: nothing left over from an earlier call
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_products_do_not_read_stale_arena_bytes(A, name, prec):
    net = _net(A, name, "he")
    ops = A.ops
    _, T = _codes(A, prec, "bf16")
    M_big = 4096
    for M in (1, 33, 257, 1000):
        res = []
        for fill in (0x00, 0xFF):
            gc.collect()
            before = dict(ops.ARENA_STATS)
            pts, g = _inputs(name, M_big, 3)
            out, dump = _forward(A, net, prec, "bf16", pts)
            delta = _chain(A, net, prec, "bf16", g, out, dump)
            _products(A, net, prec, "bf16", M_big, dump, delta)
            assert ops.ARENA_STATS["persistent"] - before["persistent"] == 3 and ops.ARENA_STATS["fresh"] == before["fresh"], \
                "the large call did not run on the arena (a dump of an earlier test is still alive?)"
            dump.fill_(fill); delta.fill_(fill)
            ops.scratch(("wgrad", net.id), A.lib.nerf_amd_weight_grads_workspace_bytes(net.id, T, M_big), dump.device).fill_(fill)
            del dump, delta, out
            before = dict(ops.ARENA_STATS)
            pts, g = _inputs(name, M, 11 + M)
            out, dump = _forward(A, net, prec, "bf16", pts)
            delta = _chain(A, net, prec, "bf16", g, out, dump)
            grads = _products(A, net, prec, "bf16", M, dump, delta)
            after = dict(ops.ARENA_STATS)
            assert after["persistent"] - before["persistent"] == 3 and after["grown"] == before["grown"] and after["fresh"] == before["fresh"], (before, after)
            _, deltas, head, _ = _read(A, net, prec, "bf16", M, dump, delta)
            res.append([out.clone()] + [deltas[L] for L in net.order] + [head] + [grads[k].clone() for k in sorted(grads)])
            del dump, delta
        for a, b in zip(*res):
            assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), (name, prec, M)


# ------------------------------------------------------------------------------------------------ 3: fp8 dumps
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_fp8_delta_slots_are_the_rounded_bf16_slots(A, name):
    """the contract test_fp8_activation_dump_is_the_rounded_bf16_dump states for activations, for every hidden delta slot"""
    net = _net(A, name, "he")
    for M in (257, 1000):
        pts, g = _inputs(name, M, 21)
        out, dump16 = _forward(A, net, "bf16", "bf16", pts)
        delta16 = _chain(A, net, "bf16", "bf16", g, out, dump16)
        out8, dump8 = _forward(A, net, "bf16", "fp8", pts)
        delta8 = _chain(A, net, "bf16", "fp8", g, out8, dump8)
        assert torch.equal(out, out8)
        assert torch.equal(_slot_rows(A, net, "bf16", "fp8", M, delta8, net.head_slot, 16), _slot_rows(A, net, "bf16", "bf16", M, delta16, net.head_slot, 16))
        for L in net.order:
            width = net.width[L]
            want = _slot_rows(A, net, "bf16", "bf16", M, delta16, L, width).float().view(M, width // 16, 16)
            got = _slot_rows(A, net, "bf16", "fp8", M, delta8, L, width).float().view(M, width // 16, 16)
            grp = want.abs().amax(-1, keepdim=True)
            err = (got - want).abs()
            assert bool((err <= grp * (2.0 ** -4) + 1e-30).all()), (name, M, L, float((err / (grp + 1e-30)).max()))
            big = want.abs() >= grp * 0.25
            rel = (err / want.abs().clamp_min(1e-30))[big & (want != 0)]
            assert rel.numel() == 0 or float(rel.max()) <= 2.0 ** -4 + 1e-6, (name, M, L, float(rel.max()))


@pytest.mark.parametrize("name", ["prop", "mip"])
def test_fp8_products_contract_the_decoded_operands(A, name):
    """with fp8 dumps the products' operands are the decoded e4m3 values (exact in bf16): same fp64 contraction, same bound"""
    net = _net(A, name, "he")
    dense, comb = {}, {}
    M = 1000
    pts, g = _inputs(name, M, 31)
    out, dump = _forward(A, net, "bf16", "fp8", pts)
    delta = _chain(A, net, "bf16", "fp8", g, out, dump)
    grads = _products(A, net, "bf16", "fp8", M, dump, delta)
    acts, deltas, head, enc = _read(A, net, "bf16", "fp8", M, dump, delta)
    _check_grads(A, net, "bf16", acts, deltas, head, enc, grads, dense, "%s bf16 fp8-dumps dense M=%d" % (name, M))
    del dump, delta
    _comb_case(A, net, "bf16", "fp8", 1000, comb)
    _emit("bwd-layers %s bf16 fp8-dumps he dense" % name, dense)
    _emit("bwd-layers %s bf16 fp8-dumps he comb" % name, comb)


# ------------------------------------------------------------------------------------------------ 4: the comparators bite
def _comb_run(A, net, M):
    pts, g_full = _inputs(net.name, M, 55)
    probes = R.comb_runs(M, 256)[0]
    idx = torch.tensor(probes, device="cuda")
    g = torch.zeros_like(g_full)
    g[idx] = g_full[idx]
    out, dump = _forward(A, net, "bf16", "bf16", pts)
    delta = _chain(A, net, "bf16", "bf16", g, out, dump)
    return pts, g, idx, out, dump, delta


@pytest.mark.parametrize("name", ["prop", "mip"])
def test_negative_controls_on_the_delta_dump(A, name):
    """One flipped sign bit / one zeroed 32-sample subtile in a CLONE of the delta dump: the products of the clone against the reference
    built from the unmodified rows must be reported, and the report must name the tensor that reads the slot."""
    net = _net(A, name, "he")
    M, slot = 1000, 2
    pts, g, idx, out, dump, delta = _comb_run(A, net, M)
    acts, deltas, head, enc = _read(A, net, "bf16", "bf16", M, dump, delta)
    _check_grads(A, net, "bf16", acts, deltas, head, enc, _products(A, net, "bf16", "bf16", M, dump, delta), {}, "unmodified", rows=idx)
    _, ls = _geometry("bf16", M)
    m = int(idx[len(idx) // 2])
    f = int(deltas[slot][m].float().abs().argmax())
    assert float(deltas[slot][m, f]) != 0.0
    # (i) one sign bit
    bad = delta.clone()
    bad[R.dump_element_offset(ls, slot, m, f) + 1] ^= 0x80
    rows = A.ops.train_dump_rows(bad, net.id, A.ops.BF16, M, slot, 256)
    diff = torch.nonzero(rows != deltas[slot])
    assert diff.tolist() == [[m, f]] and float(rows[m, f]) == -float(deltas[slot][m, f])
    with pytest.raises(AssertionError, match=r"\bw%d \(" % slot):
        _check_grads(A, net, "bf16", acts, deltas, head, enc, _products(A, net, "bf16", "bf16", M, dump, bad), {}, "sign flipped", rows=idx)
    # (ii) one whole subtile of the slot
    bad = delta.clone()
    s = m // 32
    bad[slot * ls + s * 16 * 1024: slot * ls + (s + 1) * 16 * 1024] = 0
    rows = A.ops.train_dump_rows(bad, net.id, A.ops.BF16, M, slot, 256)
    assert not bool((rows[s * 32: s * 32 + 32] != 0).any()) and torch.equal(rows[: s * 32], deltas[slot][: s * 32])
    with pytest.raises(AssertionError, match=r"\bw%d \(" % slot):
        _check_grads(A, net, "bf16", acts, deltas, head, enc, _products(A, net, "bf16", "bf16", M, dump, bad), {}, "subtile zeroed", rows=idx)


@pytest.mark.parametrize("name", ["prop", "mip"])
def test_negative_control_on_the_mask_bits(A, name):
    """One flipped ReLU mask bit in a CLONE of the activation dump: the chain run on the clone, checked against the unmodified activation
    rows, must fail at exactly that element of that layer."""
    net = _net(A, name, "he")
    M, slot = 1000, 1
    pts, g, idx, out, dump, delta = _comb_run(A, net, M)
    acts, deltas, head, enc = _read(A, net, "bf16", "bf16", M, dump, delta)
    n_sub, ls = _geometry("bf16", M)
    m = int(idx[len(idx) // 3])
    f = int(deltas[slot][m].float().abs().argmax())
    assert float(acts[slot][m, f]) > 0 and float(deltas[slot][m, f]) != 0.0
    byte, bit = R.mask_bit(m, f)
    bad = dump.clone()
    assert bad.numel() == net.slots * (ls + n_sub * 1024)
    pos = net.slots * ls + slot * n_sub * 1024 + byte
    assert (int(bad[pos]) >> bit) & 1 == 1                                  # the unit was on: the forward set its bit
    bad[pos] ^= (1 << bit)
    delta_bad = _chain(A, net, "bf16", "bf16", g, out, bad)
    deltas_bad = {L: _slot_rows(A, net, "bf16", "bf16", M, delta_bad, L, net.width[L]) for L in net.order}
    w, fold = net.operands(A, "bf16")
    for L in net.order:
        d_in, wmat = R.stage(net.name, L, head, deltas_bad, w, fold[1] if fold else None)
        rep = R.check_chain_layer(deltas_bad[L], d_in, wmat, acts[L], "bf16")
        if L != slot:
            R.assert_chain_layer("layer %d" % L, rep)
            continue
        assert rep["where"] == (m, f) and rep["worst"] > 1.0 and rep["on_zero"] == 1, rep
        with pytest.raises(AssertionError):
            R.assert_chain_layer("layer %d" % L, rep)
