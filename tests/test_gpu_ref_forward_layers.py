"""The fused Ref-NeRF forward (`ref_kernel`, nerf_amd/csrc/mlp_kernels.hip; pack_ref, pack_kernels.hip) pinned stage by stage against fp64
on its own dumps -- what tests/test_gpu_forward_layers.py does for the proposal and MipNeRF networks.

tests/ref_forward_ref.py holds the references and the derivation of every bound, tests/forward_ref.py the unpacker (RefLayout, segment
kind 'ide', the IDE table); tests/test_ref_forward_ref_host.py shows on the CPU that the comparators pass an honest emulation and report
eleven planted faults.

  1. the packed blob read back: every layer equals the rounded master bit for bit (H = [bottle_neck ; the 11 head rows]), every padding
     element and padding bias is zero, the IDE table is the one passed; also with all-distinct weights and after an in-place update;
  2. every stage of ops.ref_forward_train -- 16 hidden slots, the bottle-neck with its noise, the head rows and the spec rows in aux,
     the normal, the 39 directional inputs, rgb, the position slot, the mask records, aux's padding and the density copy -- at the tile
     edges and at a count that gives every workgroup more than one tile; no noise / a noise tensor / in-kernel Philox noise; both flags;
     one contracted case; a third weight set whose heads vary (coverage asserted on the dumped aux);
  3. the rows m >= M of the last tile are copies of row M - 1 in every slot, and nothing is written behind row M of aux, rgbo, normal;
  4. ops.ref_forward (eval, and with a noise tensor) returns the training forward's rgbo and normal bit for bit;
  5. negative controls on a real dump: one flipped sign in slot 12, one zeroed subtile of slot 8, one flipped mask bit, one aux head
     value off by 2^-10 must each be reported.

max(err / tol) of every (precision, weights, stage) goes through conftest.gate (limit 1; exact stages: violations, limit 0)."""
import ctypes
import time

import pytest
import torch

import backward_ref as R
import forward_ref as F
import ref_forward_ref as RR
import weights as W
from conftest import gate
from test_gpu_forward_layers import BF16_PERIOD, _distinct, _same_bits

pytestmark = pytest.mark.gpu

BASE_M = (1, 31, 33, 255, 256, 257, 1000)
LAY = F.LAYOUTS["ref"]
NOISE_STD, NOISE_SEED = 0.1, 0x5EED1234ABCD
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import ops
    from nerf_amd import _lib
    from nerf_amd.ref_func import ide_table

    class NS:
        pass
    ns = NS()
    ns.pkg, ns.ops, ns.lib, ns.net_id = nerf_amd, ops, _lib.lib, _lib.NET_REF
    n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
    assert ns.lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
    ns.n_cu = int(n_cu.value)
    ns.table = ide_table(4).cuda().contiguous()
    ns.nets = {}
    return ns


def _code(A, prec):
    return A.ops.BF16 if prec == "bf16" else A.ops.F32


# ------------------------------------------------------------------------------------------------ masters
def _masters(A, tag, prec):
    """the 20 + 20 tensors pack_ref takes; 'arange': all-distinct values in every weight, bias and the IDE table"""
    sd = RR.varied_state() if tag == "varied" else W.ref_state("he" if tag == "arange" else tag)
    ws, bs = RR.kernel_tensors(sd, A.table.cpu())
    if tag == "arange":
        ws = [_distinct(w.shape, 1009 * l, prec, False) for l, w in enumerate(ws[:19])] + [((torch.arange(171) + 1).float() * 2.0 ** -10).reshape(9, 19)]
        bs = [((torch.arange(b.numel()) + 1 + 300 * l).float() * 2.0 ** -6) for l, b in enumerate(bs)]
    return [w.cuda().contiguous() for w in ws], [b.cuda().contiguous() for b in bs]


class Net:
    def __init__(self, A, tag):
        self.tag = tag
        self.ws, self.bs = _masters(A, tag, "fp32")
        self.blobs, self.unpacked = {}, {}

    def packed(self, A, prec):
        if prec not in self.blobs:
            self.blobs[prec] = A.ops.pack_weights(A.net_id, _code(A, prec), self.ws, self.bs)
        return self.blobs[prec]

    def operands(self, A, prec):
        if prec not in self.unpacked:
            self.unpacked[prec] = F.unpack(self.packed(A, prec), LAY, prec)
        return self.unpacked[prec]


def _net(A, tag):
    if tag not in A.nets:
        A.nets[tag] = Net(A, tag)
    return A.nets[tag]


def _emit(prefix, worst, detail=None):
    """one gate line per stage; every line is written before the first failure is raised"""
    failed = []
    for k in sorted(worst):
        try:
            gate("%s %s %s" % (prefix, k, "violations" if k in RR.EXACT else "max(err/tol)"), worst[k], RR.limit(k))
        except AssertionError as e:
            failed.append(str(e) + ("   [%s]" % (detail[k],) if detail and k in detail else ""))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ 1: the blob
def _check_blob(prec, ws, bs, blob, what):
    u = F.unpack(blob, LAY, prec)
    mats, biases = F.layer_masters(LAY, ws, bs)
    for l in range(LAY.N_LAYERS):
        assert not bool((u.pad[l] != 0).any()), "%s: layer %d has a nonzero padding element" % (what, l)
        assert not bool((u.bpad[l] != 0).any()), "%s: layer %d has a nonzero padding bias" % (what, l)
        assert u.w[l].shape == mats[l].shape and torch.equal(u.w[l].double(), R.operand(mats[l], prec)), "%s: layer %d differs from its master" % (what, l)
        assert torch.equal(u.b[l], biases[l]), "%s: bias %d differs from its master" % (what, l)
    assert u.tail.numel() == 0 and LAY.USED_FRAGS == LAY.N_FRAGS                 # the Ref-NeRF stream has no unused fragment
    assert torch.equal(u.ide, ws[19]), what + ": the IDE table is not the one passed"
    return u


@pytest.mark.parametrize("tag", ["small", "he", "arange"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_packed_blob_reads_back_as_the_masters(A, prec, tag):
    ws, bs = _masters(A, tag, prec)
    if tag == "arange":
        for l, w in enumerate(ws[:19]):                      # the premise: exact in the stream's type, and as distinct as stated
            assert torch.equal(R.operand(w, prec), w.double()) and bool(torch.isfinite(w).all())
            flat = w.reshape(-1) if prec == "fp32" else w.reshape(-1)[: BF16_PERIOD[False]]
            assert flat.unique().numel() == flat.numel()
    blob = A.ops.pack_weights(A.net_id, _code(A, prec), ws, bs)
    assert blob.numel() == LAY.packed_bytes(prec)
    _check_blob(prec, ws, bs, blob, "ref %s %s" % (prec, tag))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_repacked_blob_follows_an_in_place_update(A, prec):
    """a spatial tensor (S2), a directional tensor (D2 = tensor 12) and the heads (tensor 9: the second row segment of layer H)"""
    ws, bs = _masters(A, "he", prec)
    before = _check_blob(prec, ws, bs, A.ops.pack_weights(A.net_id, _code(A, prec), ws, bs), "ref %s he" % prec)
    touched = [2, 12, 9]
    for t in touched:
        ws[t].mul_(-0.75).add_(0.003)
        bs[t].add_(0.125)
    after = _check_blob(prec, ws, bs, A.ops.pack_weights(A.net_id, _code(A, prec), ws, bs), "ref %s he updated" % prec)
    for l, src in enumerate(LAY.src):
        same = torch.equal(before.w[l], after.w[l]) and torch.equal(before.b[l], after.b[l])
        assert same == (src not in touched and src != "H"), (prec, l, src)
    assert torch.equal(before.w[8][:128], after.w[8][:128]) and torch.equal(before.b[8][:128], after.b[8][:128])     # bottle_neck itself: untouched
    assert not torch.equal(before.w[8][128:], after.w[8][128:]) and torch.equal(before.ide, after.ide)


# ------------------------------------------------------------------------------------------------ 2: the stages
def _inputs(M, seed):
    """positions N(0, 1.5), unit directions (the host test's inputs)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(M, 3, generator=gen) * 1.5
    d = torch.randn(M, 3, generator=gen)
    return torch.cat((x, d / d.norm(dim=1, keepdim=True)), -1).cuda().contiguous()


def _wide(pts):
    """every other position x 4 (outside the unit ball), the others x 1/4, sample 0 on the unit sphere to within rounding"""
    pts = pts.clone()
    pts[:, :3] *= torch.where(torch.arange(pts.shape[0], device=pts.device) % 2 == 1, 4.0, 0.25)[:, None]
    pts[0, :3] = torch.tensor([0.6, 0.8, 0.0], device=pts.device)
    return pts


def _forward_train(A, net, prec, pts, mode, flags, contract=False):
    """-> (rgbo, normal, dump, aux, the noise the reference adds).  mode: 'none' | 'tensor' | 'philox'"""
    M = pts.shape[0]
    noise, kw, ref_noise = None, {}, None
    if mode == "tensor":
        noise = ref_noise = (torch.randn(M, 128, generator=torch.Generator().manual_seed(7 + M)) * NOISE_STD).cuda()
    elif mode == "philox":
        kw = dict(noise_std=NOISE_STD, noise_seed=NOISE_SEED)
        ref_noise = A.ops.philox_normal(M, NOISE_STD, NOISE_SEED)
    rgbo, normal, dump, aux = A.ops.ref_forward_train(net.packed(A, prec), _code(A, prec), pts, noise, flags, contract=contract, **kw)
    return rgbo, normal, dump, aux, ref_noise


def _read(A, prec, M, dump, n=None, masks=True):
    """-> (acts {slot: rows}, slot 8 rows (n, 240), mask rows {slot: bool}) of the first n (default M) rows of a dump of M samples"""
    n = M if n is None else n
    assert F.geometry(prec, n) == F.geometry(prec, M)
    P = _code(A, prec)
    acts = {L: A.ops.train_dump_rows(dump, A.net_id, P, n, L, 256) for L in RR.HIDDEN_SLOTS}
    s8 = A.ops.train_dump_rows(dump, A.net_id, P, n, 8, RR.SLOT8_WIDTH)
    m = {L: F.mask_rows(F.mask_block(dump, "ref", prec, M, L), 256)[:n] for L in RR.HIDDEN_SLOTS} if masks else None
    return acts, s8, m


def _check_run(A, net, prec, pts, out, flags, contract, worst, detail, what):
    rgbo, normal, dump, aux, ref_noise = out
    M = pts.shape[0]
    acts, s8, masks = _read(A, prec, M, dump)
    run = {"acts": acts, "s8": s8, "aux": aux, "rgbo": rgbo.reshape(M, 4), "normal": normal.reshape(M, 3), "masks": masks}
    rep = RR.check_forward(prec, net.operands(A, prec), run, pts, ref_noise, flags, contract)
    for k, v in RR.ratios(rep).items():
        if k not in worst or v > worst[k]:
            worst[k], detail[k] = v, "%s at %s" % (what, rep[k]["where"])
    return rep


MODES = ("none", "tensor", "philox")


def _cases(A, prec, tag):
    """(M, noise mode, flags): every tile edge with one combination (rotating), all six combinations at M = 1000, and -- he weights
    only -- one count at which every persistent workgroup runs more than one tile (the weight ring, the stash and the bias table carry
    state across tiles)"""
    cases = [(M, MODES[i % 3], i % 2) for i, M in enumerate(BASE_M[:-1])]
    cases += [(1000, mode, flags) for mode in MODES for flags in (0, 1)]
    if tag == "he":
        cases.append((2 * A.n_cu * F.TILE[prec] + 77, "philox", 1))
    return cases


@pytest.mark.parametrize("tag", ["small", "he", "varied"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ref_forward_stages_against_their_own_inputs(A, prec, tag):
    net = _net(A, tag)
    worst, detail = {}, {}
    t0 = time.time()
    cases = _cases(A, prec, tag)
    for M, mode, flags in cases:
        pts = _inputs(M, 1000 + M % 997)
        out = _forward_train(A, net, prec, pts, mode, flags)
        _check_run(A, net, prec, pts, out, flags, False, worst, detail, "M=%d %s flags=%d" % (M, mode, flags))
        if tag == "varied" and M == 1000 and mode == "none" and flags == 0:
            cov = RR.coverage(out[3])                         # the element-wise stages are only exercised if the heads vary: a condition
            assert all(cov.values()), "the varied weight set does not cover: %s" % [k for k, v in cov.items() if not v]
        del out
    torch.cuda.synchronize()
    print("ref forward stages %s %s: %d runs up to M = %d in %.1f s" % (prec, tag, len(cases), max(c[0] for c in cases), time.time() - t0))
    _emit("ref-fwd-layers %s %s" % (prec, tag), worst, detail)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ref_forward_stages_contracted(A, prec):
    """the scene contraction is a flag of the sample fetch: the position slot is checked against the contracted fp64 position"""
    net = _net(A, "he")
    pts = _wide(_inputs(1000, 23))
    worst, detail = {}, {}
    out = _forward_train(A, net, prec, pts, "tensor", 0, contract=True)
    plain = _forward_train(A, net, prec, pts, "tensor", 0)
    assert not torch.equal(out[0], plain[0])                                      # the contraction is really on
    rep = _check_run(A, net, prec, pts, plain, 0, True, {}, {}, "plain dump judged as contracted")
    assert "position" in RR.failing(rep)                                          # ... and the comparator tells the two apart
    del plain
    _check_run(A, net, prec, pts, out, 0, True, worst, detail, "contracted M=1000")
    _emit("ref-fwd-layers %s he contracted" % prec, worst, detail)


# ------------------------------------------------------------------------------------------------ 3: padding rows, guard rows
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_padding_rows_are_copies_and_nothing_is_written_behind_row_m(A, prec):
    """Rows m >= M of the last tile: every lane stores its register groups unconditionally and the sample fetch (the noise fetch and the
    Philox key too) clamps m to M - 1, so the rows up to the end of the last TILE are copies of row M - 1 -- in every hidden slot and in
    ALL of slot 8 (bottle-neck with noise, directional inputs, position slot); the Ref-NeRF backward contracts whole 32-sample subtiles
    and relies on them being written and finite.  aux, rgbo and normal are per-sample outputs: nothing may be written behind row M.
    The kernel is called on buffers of this test: the dump pre-filled with 0xFF (NaN in both element types), the outputs with guard rows."""
    net = _net(A, "he")
    ops, P, G = A.ops, _code(A, prec), 64
    bad = []
    for i, M in enumerate((1, 33, 257, 1000)):
        mode, flags = MODES[i % 3], i % 2
        pts = _inputs(M, 1000 + M % 997)
        want = _forward_train(A, net, prec, pts, mode, flags)
        dump = torch.full((A.lib.nerf_amd_train_dump_bytes(A.net_id, P, M),), 0xFF, dtype=torch.uint8, device="cuda")
        assert dump.numel() == want[2].numel()
        rgbo, normal, aux = (torch.full((M + G, w), SENTINEL, device="cuda") for w in (4, 3, 16))
        s = ops._samples_pts(pts, 6, False)
        if mode == "philox":
            ops.check(A.lib.nerf_amd_ref_forward_train_dump_rng(ops._ptr(net.packed(A, prec)), P, ctypes.byref(s), flags, NOISE_SEED, None, NOISE_STD,
                                                                ops._ptr(rgbo), ops._ptr(normal), ops._ptr(dump), ops._ptr(aux), ops._stream()), "ref train rng")
        else:
            ops.check(A.lib.nerf_amd_ref_forward_train_dump(ops._ptr(net.packed(A, prec)), P, ctypes.byref(s), flags, ops._ptr(want[4]), ops._ptr(rgbo),
                                                            ops._ptr(normal), ops._ptr(dump), ops._ptr(aux), ops._stream()), "ref train")
        what = "%s M=%d %s" % (prec, M, mode)
        for name, t, w in (("rgbo", rgbo, want[0]), ("normal", normal, want[1]), ("aux", aux, want[3])):
            if not bool((t[M:] == SENTINEL).all()):
                bad.append("%s: %s is written behind row M" % (what, name))
            if not torch.equal(t[:M].reshape(-1).view(torch.int32), w.reshape(-1).view(torch.int32)):
                bad.append("%s: %s differs from ops.ref_forward_train's" % (what, name))
        tile = F.TILE[prec]
        Mpad = (M + tile - 1) // tile * tile
        acts, s8, masks = _read(A, prec, M, dump, Mpad)
        acts0, s80, _ = _read(A, prec, M, want[2], M, masks=False)
        for L, rows, rows0 in [(L, acts[L], acts0[L]) for L in RR.HIDDEN_SLOTS] + [(8, s8, s80)]:
            if not torch.equal(rows[:M].reshape(-1).view(torch.int16 if prec == "bf16" else torch.int32),
                               rows0.reshape(-1).view(torch.int16 if prec == "bf16" else torch.int32)):
                bad.append("%s: slot %d differs from ops.ref_forward_train's" % (what, L))
            if not bool(torch.isfinite(rows[M - 1].float()).all()) or not bool((rows[M:] == rows[M - 1]).all()):
                bad.append("%s: slot %d, rows m >= M are not copies of a finite row M - 1" % (what, L))
        for L in RR.HIDDEN_SLOTS:
            if not torch.equal(masks[L], acts[L] > 0):
                bad.append("%s: slot %d, mask bits of the rows m >= M" % (what, L))
        del want
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ 4: the other entry points
@pytest.mark.parametrize("tag", ["small", "he", "varied"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_eval_forward_equals_the_training_forward_bit_for_bit(A, prec, tag):
    """ops.ref_forward is other code (bf16: the wide tile with the paired prologue against the training forward's 8-wave narrow tile; no
    dump, no mask records, no aux) with the same arithmetic.  Also with a noise tensor (nerf_amd_ref_forward_train without the dump)."""
    net = _net(A, tag)
    P = _code(A, prec)
    for M in BASE_M:
        pts = _inputs(M, 1000 + M % 997)
        for flags in (0, 1):
            what = "ref %s %s M=%d flags=%d" % (prec, tag, M, flags)
            rgbo, normal, dump, aux, _ = _forward_train(A, net, prec, pts, "none", flags)
            del dump
            got = A.ops.ref_forward(net.packed(A, prec), P, pts, flags=flags)
            _same_bits(got[0], rgbo, what + ": eval rgbo against the training forward")
            _same_bits(got[1], normal, what + ": eval normal against the training forward")
            rgbo, normal, dump, aux, noise = _forward_train(A, net, prec, pts, "tensor", flags)
            del dump
            got = A.ops.ref_forward(net.packed(A, prec), P, pts, noise=noise, flags=flags)
            _same_bits(got[0], rgbo, what + ": rgbo with a noise tensor, without the dump")
            _same_bits(got[1], normal, what + ": normal with a noise tensor, without the dump")


# ------------------------------------------------------------------------------------------------ 5: the comparators bite
def test_negative_controls_on_a_real_dump(A):
    """One flipped sign bit in slot 12, one zeroed 32-sample subtile of slot 8, one flipped mask bit, one aux head value off by 2^-10, each
    in a CLONE of a real run: the same comparators must report each, at the stage that writes it and at the stages that read it."""
    net = _net(A, "he")
    prec, M = "bf16", 1000
    pts = _inputs(M, 55)
    rgbo, normal, dump, aux, noise = _forward_train(A, net, prec, pts, "tensor", 0)
    u = net.operands(A, prec)

    def check(dump_, aux_):
        acts, s8, masks = _read(A, prec, M, dump_)
        run = {"acts": acts, "s8": s8, "aux": aux_, "rgbo": rgbo, "normal": normal, "masks": masks}
        return run, RR.check_forward(prec, u, run, pts, noise, 0)
    run0, rep = check(dump, aux)
    RR.assert_forward("unmodified", rep)
    n_sub, ls = F.geometry(prec, M)
    m, slot = 613, 12
    f = int(run0["acts"][slot][m].float().argmax())
    assert float(run0["acts"][slot][m, f]) > 0
    # (i) one sign bit in slot 12 = D3's output, D4's hidden input
    bad = dump.clone()
    bad[R.dump_element_offset(ls, slot, m, f) + 1] ^= 0x80
    run, rep = check(bad, aux)
    assert torch.nonzero(run["acts"][slot] != run0["acts"][slot]).tolist() == [[m, f]]
    assert set(RR.failing(rep)) == {"D3", "D4", "mask"} and rep["D3"]["where"] == (m, f) and rep["D4"]["where"][0] == m, RR.failing(rep)
    assert rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (slot, m, f)
    with pytest.raises(AssertionError, match="D3"):
        RR.assert_forward("sign flipped", rep)
    # (ii) one whole subtile of slot 8: the bottle-neck, the directional inputs and the position slot of 32 samples
    bad = dump.clone()
    s = m // 32
    bad[8 * ls + s * 16 * 1024: 8 * ls + (s + 1) * 16 * 1024] = 0
    run, rep = check(bad, aux)
    assert not bool((run["s8"][s * 32: s * 32 + 32] != 0).any()) and torch.equal(run["s8"][: s * 32], run0["s8"][: s * 32])
    failing = set(RR.failing(rep))
    assert {"bottleneck", "ide", "ndot", "position", "S0", "S4", "D0", "D4"} <= failing, failing
    assert all(rep[k]["where"][0] // 32 == s for k in failing), {k: rep[k]["where"] for k in failing}
    # (iii) one mask bit
    bad = dump.clone()
    byte, bit = R.mask_bit(m, f)
    pos = RR.N_SLOTS * ls + slot * n_sub * 1024 + byte
    assert (int(bad[pos]) >> bit) & 1 == 1                                   # the unit was on: the forward set its bit
    bad[pos] ^= (1 << bit)
    run, rep = check(bad, aux)
    assert RR.failing(rep) == ["mask"] and rep["mask"]["worst"] == 1.0 and rep["mask"]["where"] == (slot, m, f)
    # (iv) one head value of aux (the diffuse pre-activation of channel 1) off by 2^-10
    bad_aux = aux.clone()
    bad_aux[m, 5] += 2.0 ** -10
    run, rep = check(dump, bad_aux)
    assert "heads" in RR.failing(rep) and rep["heads"]["where"] == (m, 5) and set(RR.failing(rep)) <= {"heads", "rgb"}, RR.failing(rep)
    with pytest.raises(AssertionError, match="heads"):
        RR.assert_forward("aux perturbed", rep)
