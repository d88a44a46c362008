"""The fused MLP forward (nerf_amd/csrc/mlp_kernels.hip, mlp_core.h, pack_kernels.hip) pinned layer by layer against fp64 on its own dumps.

tests/forward_ref.py holds the unpacker, the fp64 references and the derivation of every bound; tests/test_forward_ref_host.py shows on
the CPU that the comparators pass an honest emulation and report seven planted faults.

  1. the packed blob read back: every plain layer of all four layouts equals the rounded master bit for bit, every padding element and
     padding fragment is zero, the biases are the masters', the fp32 fold is within its chain bound of fp64 and the stream's folded
     operand is that fold (rounded to nearest even in bf16), also with all-distinct weights and after an in-place update;
  2. every hidden slot, the sigma head / proposal density and the rgb output of proposal_forward_train / mip_forward_train against
     fp64 on the dumped inputs and the UNPACKED operands (the blob is what the kernel multiplies), element by element without
     exemptions; the ReLU mask records against [dumped activation > 0]; the rows m >= M of the last tile;
     the integrated-PE and the contracted instantiations through the same checks;
  3. the render kernels (wide tile, resident weights) and the fp8-dump training forwards return the training forward's output bit for bit;
  4. negative controls on a real dump: one flipped sign, one zeroed subtile, one flipped mask bit must be reported.

max(err / tol) of every (network, precision, weights, stage) goes through conftest.gate (limit 1; mask records: wrong bits, limit 0)."""
import ctypes
import time

import pytest
import torch

import backward_ref as R
import forward_ref as F
import weights as W
from conftest import gate

pytestmark = pytest.mark.gpu

BASE_M = (1, 31, 33, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import ops
    from nerf_amd import _lib

    class NS:
        pass
    ns = NS()
    ns.pkg, ns.ops, ns.lib = nerf_amd, ops, _lib.lib
    ns.ids = {"prop": _lib.NET_PROPOSAL, "mip": _lib.NET_MIP, "prop128": _lib.NET_PROPOSAL_128, "mip128": _lib.NET_MIP_128}
    n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
    assert ns.lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
    ns.n_cu = int(n_cu.value)
    ns.nets = {}
    return ns


def _code(A, prec):
    return A.ops.BF16 if prec == "bf16" else A.ops.F32


# ------------------------------------------------------------------------------------------------ masters
BF16_PERIOD = {False: 65023, True: 15871}


def _distinct(shape, base, prec, narrow):
    """all-distinct, arange-based values.  fp32: the integers base + 1 .. base + n scaled by 2^-10 (exact, every one different).
    bf16 has fewer finite values than a 256 x 256 layer has elements, so there the values are bit patterns sign | magnitude taken in
    arange order with the longest period the type allows: the 65 023 normal patterns 0x0080 + k (2^-126 <= |w| < 2^128) for the plain
    layers; for the two tensors of the fold (narrow), whose products have to stay finite in fp32, the 15 871 patterns 0x3000 + k
    (2^-31 <= |w| < 2^31).  Exact in bf16 by construction, distinct inside every window of one period, and neither period is a
    multiple of a row length or a fragment size of the layouts."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64) + base
    if prec == "fp32":
        return ((i + 1).double() * 2.0 ** -10).float().reshape(shape)
    k = i % BF16_PERIOD[narrow]
    bits = ((0x3000 if narrow else 0x0080) + (k >> 1)) | ((k & 1) << 15)
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(torch.bfloat16).float().reshape(shape)


def _in_fold(name, l):
    return name.startswith("mip") and l in (7, 9)


def _masters(name, tag, prec):
    hidden = 128 if name.endswith("128") else 256
    sd = W.proposal_state("he" if tag == "arange" else tag, hidden=hidden) if name.startswith("prop") else \
        W.mip_state("he" if tag == "arange" else tag, hidden=hidden)
    ws = [v for k, v in sd.items() if k.endswith(".weight")]
    bs = [v for k, v in sd.items() if k.endswith(".bias")]
    if tag == "arange":
        ws = [_distinct(w.shape, 1009 * l, prec, _in_fold(name, l)) for l, w in enumerate(ws)]
        bs = [((torch.arange(b.numel()) + 1 + 300 * l).float() * 2.0 ** -6) for l, b in enumerate(bs)]
    return [w.cuda().contiguous() for w in ws], [b.cuda().contiguous() for b in bs]


class Net:
    def __init__(self, A, name, tag):
        self.name, self.tag, self.id, self.lay = name, tag, A.ids[name], F.LAYOUTS[name]
        self.ws, self.bs = _masters(name, tag, "fp32")
        self.blobs, self.unpacked = {}, {}

    def packed(self, A, prec):
        if prec not in self.blobs:
            self.blobs[prec] = A.ops.pack_weights(self.id, _code(A, prec), self.ws, self.bs)
        return self.blobs[prec]

    def operands(self, A, prec):
        if prec not in self.unpacked:
            self.unpacked[prec] = F.unpack(self.packed(A, prec), self.lay, prec)
        return self.unpacked[prec]


def _net(A, name, tag):
    if (name, tag) not in A.nets:
        A.nets[(name, tag)] = Net(A, name, tag)
    return A.nets[(name, tag)]


def _emit(prefix, worst, detail=None):
    """one gate line per stage; every line is written before the first failure is raised"""
    failed = []
    for k in sorted(worst):
        try:
            gate("%s %s %s" % (prefix, k, "wrong bits" if k == "mask" else "max(err/tol)"), worst[k], 0.0 if k == "mask" else 1.0)
        except AssertionError as e:
            failed.append(str(e) + ("   [%s]" % (detail[k],) if detail and k in detail else ""))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ 1: the blob
def _check_blob(A, name, prec, ws, bs, blob, what):
    """the unpacked blob against the masters.  Exact assertions raise here; -> the fold's max(err / tol) figures (MipNeRF layouts)"""
    lay = F.LAYOUTS[name]
    u = F.unpack(blob, lay, prec)
    for l, src in enumerate(lay.src):
        assert not bool((u.pad[l] != 0).any()), "%s: layer %d has a nonzero padding element" % (what, l)
        assert not bool((u.bpad[l] != 0).any()), "%s: layer %d has a nonzero padding bias" % (what, l)
        if src == "fold":
            continue
        assert torch.equal(u.w[l].double(), R.operand(ws[src], prec)), "%s: layer %d differs from its master" % (what, l)
        assert torch.equal(u.b[l], bs[src]), "%s: bias %d differs from its master" % (what, l)
    # The stream's padding fragments (PropLayout128: USED_FRAGS .. N_FRAGS): pack_proposal128 clears them with hipMemsetAsync on EVERY
    # call ("zeroed once here so that the blob is deterministic"), so what the pack guarantees is: all zero, in a fresh torch.empty blob too.
    assert u.tail.numel() == (lay.N_FRAGS - lay.USED_FRAGS) * 512 and not bool((u.tail != 0).any()), what + ": stream padding fragments"
    if not lay.fold:
        return {}
    l = lay.src.index("fold")
    assert bool(torch.isfinite(u.fold_w).all()) and bool(torch.isfinite(u.fold_b).all())
    # the stream's folded operand is the scratch fold: exactly in fp32, rounded to nearest even in bf16; its direction columns and its
    # bias are plain copies (the bias table is fp32 in both precisions)
    assert torch.equal(u.w[l][:, :256].double(), R.operand(u.fold_w, prec)), what + ": the stream's folded operand is not the scratch fold"
    assert torch.equal(u.w[l][:, 256:].double(), R.operand(ws[9][:, 256:], prec)), what + ": direction columns of the folded layer"
    assert torch.equal(u.b[l], u.fold_b), what + ": folded bias in the bias table"
    wf, tw, bf, tb = F.fold_bounds(ws[9], bs[9], ws[7], bs[7])
    return {"fold-matrix": float(((u.fold_w.double() - wf).abs() / tw).max()), "fold-bias": float(((u.fold_b.double() - bf).abs() / tb).max())}


@pytest.mark.parametrize("tag", ["small", "he", "arange"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip", "prop128", "mip128"])
def test_packed_blob_reads_back_as_the_masters(A, name, prec, tag):
    ws, bs = _masters(name, tag, prec)
    if tag == "arange":
        for l, w in enumerate(ws):                           # the premise: exact in the stream's type, and as distinct as stated
            assert torch.equal(R.operand(w, prec), w.double()) and bool(torch.isfinite(w).all())
            flat = w.reshape(-1) if prec == "fp32" else w.reshape(-1)[: BF16_PERIOD[_in_fold(name, l)]]
            assert flat.unique().numel() == flat.numel()
    blob = A.ops.pack_weights(A.ids[name], _code(A, prec), ws, bs)
    fold = _check_blob(A, name, prec, ws, bs, blob, "%s %s %s" % (name, prec, tag))
    _emit("fwd-layers %s %s %s pack" % (name, prec, tag), fold)           # (the bound is relative: it holds for the arange weights too)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip", "prop128", "mip128"])
def test_repacked_blob_follows_an_in_place_update(A, name, prec):
    """layer 0 sits in the resident prefix of the bf16 render kernels, layer 2 is streamed; for MipNeRF also the three tensors of the fold"""
    ws, bs = _masters(name, "he", prec)
    before = F.unpack(A.ops.pack_weights(A.ids[name], _code(A, prec), ws, bs), F.LAYOUTS[name], prec)
    touched = [0, 2] + ([7, 9] if name.startswith("mip") else [])
    for t in touched:
        ws[t].mul_(-0.75).add_(0.003)
        bs[t].add_(0.125)
    blob = A.ops.pack_weights(A.ids[name], _code(A, prec), ws, bs)
    fold = _check_blob(A, name, prec, ws, bs, blob, "%s %s updated" % (name, prec))
    after = F.unpack(blob, F.LAYOUTS[name], prec)
    for l, src in enumerate(F.LAYOUTS[name].src):
        same = torch.equal(before.w[l], after.w[l]) and torch.equal(before.b[l], after.b[l])
        assert same == (src not in touched and src != "fold"), (name, prec, l, src)
    _emit("fwd-layers %s %s he-updated pack" % (name, prec), fold)


# ------------------------------------------------------------------------------------------------ 2: the layers
def _inputs(name, M, seed):
    """the positions of test_gpu_backward_layers._inputs"""
    gen = torch.Generator().manual_seed(seed)
    if name == "prop":
        return (torch.rand(M, 3, generator=gen) * 2 - 1).cuda()
    return torch.cat((torch.randn(M, 3, generator=gen) * 1.5, torch.randn(M, 3, generator=gen)), -1).cuda()


def _forward_train(A, net, prec, pts, fmt="bf16", contract=False):
    T = A.ops.BF16_F8 if fmt == "fp8" else _code(A, prec)
    return (A.ops.proposal_forward_train if net.name == "prop" else A.ops.mip_forward_train)(net.packed(A, prec), T, pts, contract=contract)


def _forward(A, net, prec, pts, contract=False):
    return (A.ops.proposal_forward if net.name == "prop" else A.ops.mip_forward)(net.packed(A, prec), _code(A, prec), pts, contract=contract)


def _read(A, net, prec, M, dump, n=None):
    """-> (acts, encoding slot rows, mask rows) of the first n (default M) rows of a bf16 / fp32 dump of M samples"""
    n = M if n is None else n
    assert F.geometry(prec, n) == F.geometry(prec, M)
    P = _code(A, prec)
    width = F.WIDTH[net.name]
    acts = {L: A.ops.train_dump_rows(dump, net.id, P, n, L, width[L]) for L in range(len(width))}
    enc = A.ops.train_dump_rows(dump, net.id, P, n, F.ENC_SLOT[net.name], F.ENC_WIDTH[net.name])
    masks = {L: F.mask_rows(F.mask_block(dump, net.name, prec, M, L), width[L])[:n] for L in range(len(width))}
    return acts, enc, masks


def _check_padding_rows(A, net, prec, M, dump, what):
    """Rows m >= M of the last tile.  dump_hidden / dump_breg store every lane's register group unconditionally, and the sample fetch
    clamps m to M - 1, so the rows up to the end of the last TILE are written and are copies of row M - 1.  The backward relies on
    exactly this much: its weight-gradient products contract whole 32-sample subtiles, the chain gives the rows m >= M a zero head
    delta, and 0 x (a finite activation) adds nothing while 0 x (stale NaN bytes) would -- the rows must be written and finite.
    Asserted: they equal row M - 1 bit for bit (hence written, hence finite), in every hidden slot and the encoding slot, and their
    mask bits are [activation > 0] like everybody's.  -> the list of failures (raised by the caller after the gate lines are out)."""
    tile = F.TILE[prec]
    Mpad = (M + tile - 1) // tile * tile
    if Mpad == M:
        return []
    bad = []
    acts, enc, masks = _read(A, net, prec, M, dump, Mpad)
    for L, rows in list(acts.items()) + [("enc", enc)]:
        if not bool(torch.isfinite(rows[M - 1].float()).all()) or not bool((rows[M:] == rows[M - 1]).all()):
            bad.append("%s: slot %s, rows m >= M are not copies of a finite row M - 1" % (what, L))
    for L, m in masks.items():
        if not torch.equal(m, acts[L] > 0):
            bad.append("%s: slot %d, mask bits of the rows m >= M" % (what, L))
    return bad


def _check_run(A, net, prec, M, out, dump, worst, detail, what, padding):
    acts, enc, masks = _read(A, net, prec, M, dump)
    rep = F.check_forward(net.name, prec, net.lay, net.operands(A, prec), acts, enc, out, masks)
    for k, v in F.ratios(rep).items():
        if k not in worst or v > worst[k]:
            worst[k], detail[k] = v, "%s at %s" % (what, rep[k]["where"])
    padding += _check_padding_rows(A, net, prec, M, dump, what)


def _sample_counts(A, prec):
    return list(BASE_M) + [3 * A.n_cu * F.TILE[prec] + 77]


@pytest.mark.parametrize("tag", ["small", "he"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_forward_layers_against_their_own_inputs(A, name, prec, tag):
    """Part 2.  The sample counts cover the tile edges and one count at which every persistent workgroup runs at least three tiles
    (3 n_cu tile + 77: the weight ring and the encoding stash carry state across tiles)."""
    net = _net(A, name, tag)
    worst, detail, padding = {}, {}, []
    t0 = time.time()
    Ms = _sample_counts(A, prec)
    for M in Ms:
        pts = _inputs(name, M, 1000 + M % 997)
        out, dump = _forward_train(A, net, prec, pts)
        _check_run(A, net, prec, M, out, dump, worst, detail, "M=%d" % M, padding)
        del dump
    torch.cuda.synchronize()
    print("forward layers %s %s %s: %d sample counts up to %d in %.1f s" % (name, prec, tag, len(Ms), max(Ms), time.time() - t0))
    _emit("fwd-layers %s %s %s" % (name, prec, tag), worst, detail)
    assert not padding, "\n".join(padding)


def _ipe_samples(A, n_rays, S):
    """-> a maker of fresh sample descriptors (rays + S + 1 depths per ray, integrated PE); the closure keeps the tensors alive"""
    gen = torch.Generator().manual_seed(17 + n_rays)
    rays = torch.cat((torch.rand(n_rays, 3, generator=gen) - 0.5, torch.randn(n_rays, 3, generator=gen)), -1).cuda().contiguous()
    z = torch.sort(torch.rand(n_rays, S + 1, generator=gen) * 4 + 2, dim=-1)[0].cuda().contiguous()
    dn = A.ops.dirs_norm(rays)
    return lambda: A.ops.samples_rays(rays, S, z=z, ipe_radius=2.0 / 12.0 ** 0.5 / 55.0, ipe_dir_norm=dn)


def _wide(pts):
    """positions four times wider: most of them lie outside the unit ball, where the contraction acts"""
    pts = pts.clone()
    pts[:, :3] *= 4.0
    return pts


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_forward_layers_integrated_pe_and_contracted(A, prec):
    """The integrated-PE training forward (its own kernel instantiation, through mip_forward_train_samples) and the scene contraction
    (a flag of the sample fetch): the layer checks need only the dump.  33 rays x 32 samples = 1056: neither tile divides it."""
    net = _net(A, "mip", "he")
    P = _code(A, prec)
    n_rays, S = 33, 32
    M = n_rays * S
    make = _ipe_samples(A, n_rays, S)
    worst, detail, padding = {}, {}, []
    out, dump = A.ops.mip_forward_train_samples(net.packed(A, prec), P, make(), (n_rays, S), "cuda")
    _check_run(A, net, prec, M, out.reshape(M, 4), dump, worst, detail, "ipe M=%d" % M, padding)
    del dump
    _emit("fwd-layers mip %s he ipe" % prec, worst, detail)
    worst, detail = {}, {}
    pts = _wide(_inputs("mip", 1000, 23))
    out, dump = _forward_train(A, net, prec, pts, contract=True)
    plain, dump2 = _forward_train(A, net, prec, pts)
    assert not torch.equal(out, plain)                                        # the contraction is really on
    del dump2
    _check_run(A, net, prec, 1000, out, dump, worst, detail, "contracted M=1000", padding)
    del dump
    _emit("fwd-layers mip %s he contracted" % prec, worst, detail)
    assert not padding, "\n".join(padding)


# ------------------------------------------------------------------------------------------------ 3: render == training forward
def _same_bits(a, b, what):
    a, b = a.reshape(-1).view(torch.int32), b.reshape(-1).view(torch.int32)
    assert a.shape == b.shape and torch.equal(a, b), "%s: %d outputs differ" % (what, int((a != b).sum()) if a.shape == b.shape else -1)


def _ray_split(M):
    """M = n_rays x S for the integrated-PE descriptor: the largest S of a few that divides M (1 -> M rays of one sample)"""
    S = next(s for s in (32, 17, 11, 5, 3, 1) if M % s == 0)
    return M // S, S


@pytest.mark.parametrize("tag", ["small", "he"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_render_kernels_equal_the_training_forward_bit_for_bit(A, name, prec, tag):
    """The non-training instantiations are different code (bf16: the wide tile with resident weights against, for the proposal network,
    the 8-wave narrow tile; the integrated-PE render kernel is an instantiation of its own, without resident weights and without the
    paired prologue) with the same arithmetic: same operands, same K order, same conversions.  So are the fp8-dump forwards.  Every
    form -- plain, contracted and, for MipNeRF, integrated PE -- at every sample count."""
    net = _net(A, name, tag)
    P = _code(A, prec)
    for M in _sample_counts(A, prec):
        what = "%s %s %s M=%d" % (name, prec, tag, M)
        pts = _inputs(name, M, 1000 + M % 997)
        for contract in (False, True):
            x = _wide(pts) if contract else pts
            form = "contracted" if contract else "plain"
            out, dump = _forward_train(A, net, prec, x, contract=contract)
            del dump
            _same_bits(_forward(A, net, prec, x, contract=contract), out, "%s %s: render kernel against the training forward" % (what, form))
            if prec == "bf16":
                out8, dump8 = _forward_train(A, net, prec, x, fmt="fp8", contract=contract)
                del dump8
                _same_bits(out8, out, "%s %s: fp8-dump training forward" % (what, form))
        if name == "mip":
            n_rays, S = _ray_split(M)
            make = _ipe_samples(A, n_rays, S)
            out, dump = A.ops.mip_forward_train_samples(net.packed(A, prec), P, make(), (n_rays, S), "cuda")
            del dump
            _same_bits(A.ops.mip_forward_samples(net.packed(A, prec), P, make(), (n_rays, S), "cuda"), out,
                       what + " integrated PE (%d x %d): render kernel against the training forward" % (n_rays, S))
            if prec == "bf16":
                out8, dump8 = A.ops.mip_forward_train_samples(net.packed(A, prec), A.ops.BF16_F8, make(), (n_rays, S), "cuda")
                del dump8
                _same_bits(out8, out, what + " integrated PE: fp8-dump training forward")


# ------------------------------------------------------------------------------------------------ 4: the comparators bite
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_negative_controls_on_the_activation_dump(A, name):
    """One flipped sign bit, one zeroed 32-sample subtile, one flipped mask bit in a CLONE of a real dump: the same comparators must
    report each, at the slot that holds it and at the layer that reads it."""
    net = _net(A, name, "he")
    prec, M, slot = "bf16", 1000, 2
    pts = _inputs(name, M, 55)
    out, dump = _forward_train(A, net, prec, pts)
    u = net.operands(A, prec)
    acts, enc, masks = _read(A, net, prec, M, dump)
    F.assert_forward("unmodified", F.check_forward(name, prec, net.lay, u, acts, enc, out, masks))
    _, ls = F.geometry(prec, M)
    m = 613
    f = int(acts[slot][m].float().argmax())
    assert float(acts[slot][m, f]) > 0
    # (i) one sign bit
    bad = dump.clone()
    bad[R.dump_element_offset(ls, slot, m, f) + 1] ^= 0x80
    acts_b, enc_b, masks_b = _read(A, net, prec, M, bad)
    assert torch.nonzero(acts_b[slot] != acts[slot]).tolist() == [[m, f]] and float(acts_b[slot][m, f]) == -float(acts[slot][m, f])
    rep = F.check_forward(name, prec, net.lay, u, acts_b, enc_b, out, masks_b)
    r = F.ratios(rep)
    assert r["h2"] > 1.0 and rep["h2"]["where"] == (m, f) and r["h3"] > 1.0 and rep["h3"]["where"][0] == m, rep
    assert rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (slot, m, f)           # (the record still says "on", the element is negative)
    assert all(v <= 1.0 for k, v in r.items() if k not in ("h2", "h3", "mask")), r
    with pytest.raises(AssertionError, match="h2"):
        F.assert_forward("sign flipped", rep)
    # (ii) one whole subtile of the slot
    bad = dump.clone()
    s = m // 32
    bad[slot * ls + s * 16 * 1024: slot * ls + (s + 1) * 16 * 1024] = 0
    acts_b, enc_b, masks_b = _read(A, net, prec, M, bad)
    assert not bool((acts_b[slot][s * 32: s * 32 + 32] != 0).any()) and torch.equal(acts_b[slot][: s * 32], acts[slot][: s * 32])
    rep = F.check_forward(name, prec, net.lay, u, acts_b, enc_b, out, masks_b)
    r = F.ratios(rep)
    assert r["h2"] > 1.0 and rep["h2"]["where"][0] // 32 == s and r["h3"] > 1.0 and rep["h3"]["where"][0] // 32 == s, rep
    assert rep["mask"]["worst"] == float((acts[slot][s * 32: s * 32 + 32] > 0).sum())
    with pytest.raises(AssertionError, match="h2"):
        F.assert_forward("subtile zeroed", rep)
    # (iii) one mask bit
    bad = dump.clone()
    byte, bit = R.mask_bit(m, f)
    n_sub = F.geometry(prec, M)[0]
    pos = (F.ENC_SLOT[name] + 1) * ls + slot * n_sub * 1024 + byte
    assert (int(bad[pos]) >> bit) & 1 == 1                                   # the unit was on: the forward set its bit
    bad[pos] ^= (1 << bit)
    acts_b, enc_b, masks_b = _read(A, net, prec, M, bad)
    rep = F.check_forward(name, prec, net.lay, u, acts_b, enc_b, out, masks_b)
    assert rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (slot, m, f)
    assert all(v <= 1.0 for k, v in F.ratios(rep).items() if k != "mask")
    with pytest.raises(AssertionError, match="mask"):
        F.assert_forward("mask bit flipped", rep)
