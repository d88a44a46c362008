"""The Ref-NeRF parameter backward (bwd_ref_backward) and the density-gradient chains (bwd_density_grad), nerf_amd/csrc/bwd_kernels.hip,
pinned stage by stage against fp64 on their own inputs -- what tests/test_gpu_backward_layers.py does for the proposal and MipNeRF
backward and tests/test_gpu_ref_forward_layers.py for the Ref-NeRF forward.

tests/ref_backward_ref.py holds the references and the derivation of every bound; tests/test_ref_backward_ref_host.py shows on the CPU
that the stages compose to torch.autograd, that an honest emulation passes every comparator and that nine planted faults are reported.

The test OWNS the workspace: it calls nerf_amd_ref_backward / nerf_amd_density_grad through ctypes exactly as ops.ref_backward /
ops.density_grad do, on a tensor it allocated and pre-filled, and reads the delta dump, d_allin and d_enc out of it afterwards.

  a  spec-head delta, b  directional chain + d_allin, c  heads delta, d  spatial chain: every element, fp32 and bf16, three weight sets,
     tile edges and a count that gives every workgroup more than one tile, noise tensor / Philox noise / sRGB variants;
  e  all 20 + 20 parameter gradients, dense and with comb probes;
  f  the density-gradient chains of both networks: x_stride 3 / 6, scale absent / contiguous / strided, contracted positions;
  workspace and outputs pre-filled with 0x00 and 0xFF bytes: bit-identical results (the slot-8 memset is gone; every gradient element
     is overwritten); two calls are bit-identical (no kernel on this path accumulates with floating-point atomics);
  the entry points reject the fp8-dump precision for Ref-NeRF; ops.density_grad returns the bits of the ctypes call;
  five negative controls on copies of real dumps.

max(err / tol) of every (precision, weights, stage) goes through conftest.gate (limit 1; exact stages: violations, limit 0)."""
import ctypes
import time

import pytest
import torch

import backward_ref as R
import forward_ref as F
import ref_backward_ref as RB
import ref_forward_ref as RR
import weights as W
from conftest import gate
from test_gpu_ref_forward_layers import BASE_M, MODES, _code, _forward_train, _inputs, _masters, _read, _wide

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import _lib, ops
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


class Net:
    def __init__(self, A, tag):
        self.tag = tag
        self.ws, self.bs = _masters(A, tag, "fp32")
        self.fwd, self.bwd, self.w64 = {}, {}, {}

    def packed(self, A, prec):
        if prec not in self.fwd:
            self.fwd[prec] = A.ops.pack_weights(A.net_id, _code(A, prec), self.ws, self.bs)
        return self.fwd[prec]

    def packed_bwd(self, A, prec):
        if prec not in self.bwd:
            self.bwd[prec] = A.ops.pack_weights_backward(A.net_id, _code(A, prec), self.ws)
        return self.bwd[prec]

    def operands(self, prec):
        if prec not in self.w64:
            self.w64[prec] = RB.operands(self.ws, prec)
        return self.w64[prec]


def _net(A, tag):
    if tag not in A.nets:
        A.nets[tag] = Net(A, tag)
    return A.nets[tag]


def _filled(nbytes, fill):
    t = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device="cuda")
    off = (-t.data_ptr()) % 256
    return t[off: off + nbytes]


def _g_out(M, seed):
    return torch.randn(M, 7, generator=torch.Generator().manual_seed(seed)).cuda()


def _backward(A, net, prec, dump, aux, dirs, g_out, flags, fill=0x00, ws=None):
    """nerf_amd_ref_backward on storage of this test (`ws`: a caller's workspace, at any alignment) -> (workspace, {name: gradient})"""
    ops, P = A.ops, _code(A, prec)
    M = g_out.shape[0]
    need = A.lib.nerf_amd_ref_backward_workspace_bytes(P, M)
    assert RB.partials_offset(prec, M) < need                     # the delta dump and d_allin lie where ref_backward_ref reads them
    if ws is None:
        ws = _filled(need, fill)
        assert ws.data_ptr() % 256 == 0
    assert ws.numel() == need
    shapes = ops.REF_GRAD_SHAPES
    gw = [_filled(4 * s[0] * s[1], fill).view(torch.float32).view(s) for s in shapes]
    gb = [_filled(4 * s[0], fill).view(torch.float32) for s in shapes]
    dirs = dirs.contiguous()
    ops.check(A.lib.nerf_amd_ref_backward(ops._ptr(net.packed_bwd(A, prec)), P, int(flags), M, ops._ptr(dump), ops._ptr(aux), ops._ptr(dirs), dirs.shape[1],
                                          ops._ptr(g_out), g_out.shape[1], ops._ptr(A.table), ops._ptr_array(gw), ops._ptr_array(gb), ops._ptr(ws), ops._stream()),
              "nerf_amd_ref_backward")
    return ws, R.named_grads(gw, gb)


def _read_run(A, prec, M, out, ws, dirs, g_out):
    """everything the stages read: the activation dump's rows and mask records up to the end of the last tile, the delta dump out of
    the workspace (through nerf_amd_train_dump_to_rows with the workspace as the dump), d_allin"""
    rgbo, normal, dump, aux, _ = out
    P, Mp = _code(A, prec), RB.m_pad(prec, M)
    acts, s8, masks = _read(A, prec, M, dump, Mp)
    deltas = {L: A.ops.train_dump_rows(ws, A.net_id, P, Mp, L, 256) for L in RR.HIDDEN_SLOTS}
    s8d = A.ops.train_dump_rows(ws, A.net_id, P, Mp, 8, RB.S8D_WIDTH)
    return {"acts": {L: v[:M] for L, v in acts.items()}, "s8": s8[:M], "masks": masks, "aux": aux, "dirs": dirs, "g_out": g_out,
            "deltas": {L: v[:M] for L, v in deltas.items()}, "deltas_pad": deltas, "s8d": s8d, "d_allin": RB.dallin_rows(ws, prec, M)}


def _check_stages(A, net, prec, run, flags, worst, detail, what):
    rep = RB.check_elementwise(prec, run, A.table, flags)
    rep.update(RB.check_chains(prec, net.operands(prec), run))
    for k, v in RB.ratios(rep).items():
        if k not in worst or v > worst[k]:
            worst[k], detail[k] = v, "%s at %s" % (what, rep[k]["where"])
    return rep


def _check_grads(A, prec, run, grads, worst, what, rows=None):
    refs = RB.grad_refs(prec, run, 2 * A.n_cu, rows)              # (2 n_cu: upper bound of wgrad_workgroups for every product)
    assert sorted(refs) == sorted(grads)
    rep = R.grad_ratios(refs, grads)
    for k, v in rep.items():
        worst[k] = max(worst.get(k, 0.0), v)
    return rep


def _emit(prefix, worst, detail=None):
    """one gate line per stage / tensor; every line is written before the first failure is raised"""
    failed = []
    for k in sorted(worst):
        try:
            gate("%s %s %s" % (prefix, k, "violations" if k in RB.EXACT else "max(err/tol)"), worst[k], RB.limit(k))
        except AssertionError as e:
            failed.append(str(e) + ("   [%s]" % (detail[k],) if detail and k in detail else ""))
    assert not failed, "\n".join(failed)


def _cases(A, prec, tag):
    """(M, noise mode, flags): every tile edge with one combination (rotating), all six combinations at M = 1000, and -- he weights
    only -- one count at which every persistent workgroup of the chains runs more than one tile"""
    cases = [(M, MODES[i % 3], i % 2) for i, M in enumerate(BASE_M[:-1])]
    cases += [(1000, mode, flags) for mode in MODES for flags in (0, 1)]
    if tag == "he":
        cases.append((2 * A.n_cu * R.TILE[prec] + 77, "philox", 1))
    return cases


# ------------------------------------------------------------------------------------------------ a-e, dense
@pytest.mark.parametrize("tag", ["small", "he", "varied"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ref_backward_stages_against_their_own_inputs(A, prec, tag):
    net = _net(A, tag)
    stages, detail, prods = {}, {}, {}
    t0 = time.time()
    cases = _cases(A, prec, tag)
    for M, mode, flags in cases:
        pts = _inputs(M, 1000 + M % 997)
        out = _forward_train(A, net, prec, pts, mode, flags)
        if tag == "varied" and M == 1000 and mode == "none":
            cov = RR.coverage(out[3])
            assert all(cov.values()), "the varied weight set does not cover: %s" % [k for k, v in cov.items() if not v]
        g_out = _g_out(M, 3 + M)
        ws, grads = _backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, flags)
        run = _read_run(A, prec, M, out, ws, pts[:, 3:6], g_out)
        what = "M=%d %s flags=%d" % (M, mode, flags)
        _check_stages(A, net, prec, run, flags, stages, detail, what)
        _check_grads(A, prec, run, grads, prods, what)
        if mode != "none":                                        # the bottle-neck products contract the PERTURBED rows of slot 8
            plain = _forward_train(A, net, prec, pts, "none", flags)
            assert not torch.equal(_read(A, prec, M, plain[2], masks=False)[1][:, :128], run["s8"][:, :128])
            del plain
        del out, ws, run
    torch.cuda.synchronize()
    print("ref backward stages %s %s: %d runs up to M = %d in %.1f s" % (prec, tag, len(cases), max(c[0] for c in cases), time.time() - t0))
    _emit("ref-bwd-layers %s %s" % (prec, tag), stages, detail)
    _emit("ref-bwd-layers %s %s dense" % (prec, tag), prods)


# ------------------------------------------------------------------------------------------------ e, comb probes
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_comb_probes_products(A, prec):
    """at most 512 samples carry a gradient, one per 32-sample subtile: the bound is far below one sample's share"""
    net = _net(A, "he")
    worst = {}
    t0 = time.time()
    for M in (1, 33, 257, 1000, 70001):
        pts = _inputs(M, 77 + M % 991)
        g_full = _g_out(M, 5 + M)
        out = _forward_train(A, net, prec, pts, "tensor", 0)
        for r, probes in enumerate(R.comb_runs(M, R.TILE[prec])):
            idx = torch.tensor(probes, device="cuda")
            g_out = torch.zeros_like(g_full)
            g_out[idx] = g_full[idx]
            ws, grads = _backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, 0)
            run = _read_run(A, prec, M, out, ws, pts[:, 3:6], g_out)
            unprobed = torch.ones(RB.m_pad(prec, M), dtype=torch.bool, device="cuda")
            unprobed[idx] = False
            for L, d in list(run["deltas_pad"].items()) + [(8, run["s8d"])]:
                assert not bool((d[unprobed] != 0).any()), "%s M=%d run %d: delta slot %s is nonzero on an unprobed sample" % (prec, M, r, L)
            _check_grads(A, prec, run, grads, worst, "comb M=%d run %d" % (M, r), rows=idx)
            del ws, run
        del out
    torch.cuda.synchronize()
    print("ref backward comb %s: %.1f s" % (prec, time.time() - t0))
    _emit("ref-bwd-layers %s he comb" % prec, worst)


# ------------------------------------------------------------------------------------------------ workspace, repeatability
def _bits_of(run, grads):
    out = [RB._bits(run["deltas_pad"][L]) for L in RR.HIDDEN_SLOTS] + [RB._bits(run["s8d"]), RB._bits(run["d_allin"])]
    return out + [grads[k].view(torch.int32) for k in sorted(grads)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_nothing_is_read_before_it_is_written(A, prec):
    """The workspace and the 40 output tensors pre-filled with 0x00 and with 0xFF bytes (NaN in both element types): every gradient, every
    delta slot up to the end of the last tile and d_allin are bit-identical and finite.  That pins the removed slot-8 memset (the two
    element-wise kernels write every element the chains and products read) and that the finalize windows overwrite every element of the
    gradient tensors (ops._grad_buffers hands out torch.empty storage and clears nothing).  A third call repeats the first bit for bit:
    no kernel on this path accumulates with floating-point atomics (the products' partial sums are combined in a fixed order)."""
    net = _net(A, "he")
    for i, M in enumerate((1, 33, 257, 1000)):
        pts = _inputs(M, 11 + M)
        g_out = _g_out(M, 9 + M)
        out = _forward_train(A, net, prec, pts, MODES[i % 3], i % 2)
        res = []
        for fill in (0x00, 0xFF, 0x00):
            ws, grads = _backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, i % 2, fill)
            res.append(_bits_of(_read_run(A, prec, M, out, ws, pts[:, 3:6], g_out), grads))
        for a, b, c in zip(*res):
            assert torch.equal(a, b), (prec, M, "0x00 against 0xFF pre-fill")
            assert torch.equal(a, c), (prec, M, "second call against the first")
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_entry_points_reject_the_fp8_dump_precision_for_ref_nerf(A):
    ops, lib, F8 = A.ops, A.lib, A.ops.BF16_F8
    M = 33
    assert lib.nerf_amd_train_dump_bytes(A.net_id, F8, M) == 0 and lib.nerf_amd_ref_backward_workspace_bytes(F8, M) == 0
    assert lib.nerf_amd_density_grad_workspace_bytes(A.net_id, F8, M) == 0
    net = _net(A, "he")
    pts = _inputs(M, 1)
    out = _forward_train(A, net, "bf16", pts, "none", 0)
    g_out = _g_out(M, 1)
    ws = _filled(lib.nerf_amd_ref_backward_workspace_bytes(ops.BF16, M), 0)
    gw = [torch.zeros(s, device="cuda") for s in ops.REF_GRAD_SHAPES]
    gb = [torch.zeros(s[0], device="cuda") for s in ops.REF_GRAD_SHAPES]
    dirs = pts[:, 3:6].contiguous()
    rc = lib.nerf_amd_ref_backward(ops._ptr(net.packed_bwd(A, "bf16")), F8, 0, M, ops._ptr(out[2]), ops._ptr(out[3]), ops._ptr(dirs), 3, ops._ptr(g_out), 7,
                                   ops._ptr(A.table), ops._ptr_array(gw), ops._ptr_array(gb), ops._ptr(ws), ops._stream())
    assert rc != 0 and not any(bool((t != 0).any()) for t in gw + gb)
    grad = torch.zeros(M, 3, device="cuda")
    rc = lib.nerf_amd_density_grad(A.net_id, ops._ptr(net.packed_bwd(A, "bf16")), F8, M, ops._ptr(out[2]), ops._ptr(pts), 6, None, 0, ops._ptr(grad), ops._ptr(ws),
                                   ops._stream())
    assert rc != 0 and not bool((grad != 0).any())
    s = ops._samples_pts(pts, 6, False)
    rgbo, normal, aux = torch.zeros(M, 4, device="cuda"), torch.zeros(M, 3, device="cuda"), torch.zeros(M, 16, device="cuda")
    rc = lib.nerf_amd_ref_forward_train_dump(ops._ptr(net.packed(A, "bf16")), F8, ctypes.byref(s), 0, None, ops._ptr(rgbo), ops._ptr(normal), ops._ptr(out[2]),
                                             ops._ptr(aux), ops._stream())
    assert rc != 0


# ------------------------------------------------------------------------------------------------ f: density gradients
class PropNet:
    def __init__(self, A):
        state = W.proposal_state("he")
        self.ws = [v.cuda().contiguous() for k, v in state.items() if k.endswith(".weight")]
        self.bs = [v.cuda().contiguous() for k, v in state.items() if k.endswith(".bias")]
        self.blobs = {}

    def packed(self, A, prec):
        P = _code(A, prec)
        if prec not in self.blobs:
            self.blobs[prec] = (A.ops.pack_weights(A.ops.NET_PROPOSAL, P, self.ws, self.bs), A.ops.pack_weights_backward(A.ops.NET_PROPOSAL, P, self.ws))
        return self.blobs[prec]


def _density_call(A, net_id, blob, prec, dump, x, scale, contract, fill=0xFF):
    ops, P = A.ops, _code(A, prec)
    M = x.shape[0]
    ws = _filled(A.lib.nerf_amd_density_grad_workspace_bytes(net_id, P, M), fill)
    out = _filled(M * 12, fill).view(torch.float32).view(M, 3)
    ops.check(A.lib.nerf_amd_density_grad(net_id | (0x100 if contract else 0), ops._ptr(blob), P, M, ops._ptr(dump), ops._ptr(x), x.stride(0),
                                          ops._ptr(scale), scale.stride(0) if scale is not None else 0, ops._ptr(out), ops._ptr(ws), ops._stream()),
              "nerf_amd_density_grad")
    return ws[: M * 256].view(torch.float32).view(M, 64), out


def _scale(M, kind):
    if kind == "none":
        return None
    s = torch.rand(M, 4, generator=torch.Generator().manual_seed(M)).cuda() + 0.5
    return s[:, 0].contiguous() if kind == "contiguous" else s[:, 3]             # strided: a column of an (M, 4) gradient, as training passes it


@pytest.mark.parametrize("name", ["ref", "prop"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_density_gradient_chains(A, prec, name):
    """d_enc from the mask records alone (and against the slots the parameter chain stores under a unit density gradient), then the
    encoding's derivative against the d_enc in the workspace; ops.density_grad returns the same bits as the call made here."""
    ops, P = A.ops, _code(A, prec)
    worst, detail = {}, {}
    kinds = ("none", "contiguous", "strided")
    Ms = list(BASE_M) + [2 * A.n_cu * R.TILE[prec] + 77]
    variants = [(M, False, kinds[i % 3], 6 if i % 2 else 3) for i, M in enumerate(Ms)] + [(1000, True, k, s) for k, s in zip(kinds, (3, 6, 6))]
    if name == "ref":
        net, net_id = _net(A, "he"), A.net_id
        w = net.operands(prec)
    else:
        net, net_id = PropNet(A), ops.NET_PROPOSAL
        w = [R.operand(t, prec) for t in net.ws]
    for M, contract, kind, stride in variants:
        pts = _wide(_inputs(M, 40 + M % 89)) if contract else _inputs(M, 40 + M % 89)
        x = pts if stride == 6 else pts[:, :3].contiguous()
        if name == "ref":
            out = ops.ref_forward_train(net.packed(A, prec), P, pts, None, 0, contract=contract)
            dump, blob = out[2], net.packed_bwd(A, prec)
            unit = torch.zeros(M, 7, device="cuda")
            unit[:, 3] = 1.0
            wsb, _ = _backward(A, net, prec, dump, out[3], pts[:, 3:6], unit, 0)
            deltas = {L: ops.train_dump_rows(wsb, net_id, P, M, L, 256) for L in (4, 0)}
            masks = {L: F.mask_rows(F.mask_block(dump, "ref", prec, M, L), 256) for L in range(8)}
        else:
            fwd, blob = net.packed(A, prec)
            _, dump = ops.proposal_forward_train(fwd, P, pts[:, :3].contiguous(), contract=contract)
            delta = ops.proposal_backward_chain(blob, P, torch.ones(M, device="cuda"), dump)
            deltas = {0: ops.train_dump_rows(delta, net_id, P, M, 0, 256)}
            masks = {L: F.mask_rows(F.mask_block(dump, "prop", prec, M, L), 256) for L in range(4)}
        scale = _scale(M, kind)
        d_enc, got = _density_call(A, net_id, blob, prec, dump, x, scale, contract)
        rep = RB.check_density_grad(name, prec, w, masks if M <= 4096 else None, d_enc, pts[:, :3], scale, contract, got, deltas)
        what = "M=%d contract=%d scale=%s stride=%d" % (M, contract, kind, stride)
        for k, v in RB.ratios(rep).items():
            if k not in worst or v > worst[k]:
                worst[k], detail[k] = v, "%s at %s" % (what, rep[k]["where"])
        public = ops.density_grad(net_id, blob, P, dump, x, scale=scale, contract=contract)
        assert torch.equal(public.view(torch.int32), got.view(torch.int32)), what + ": ops.density_grad differs from the ctypes call"
        if contract:
            plain = RB.pe_grad_ref(d_enc, pts[:, :3], scale, False)
            assert float(((got.double() - plain[0]).abs() / plain[1]).max()) > 1.0          # ... and the flag matters to the comparator
            r = pts[:, :3].norm(dim=1)
            assert float(r.min()) < 1.0 < float(r.max())
        del dump
    _emit("ref-bwd-layers %s density-grad %s" % (prec, name), worst, detail)


# ------------------------------------------------------------------------------------------------ the comparators bite
def test_negative_controls_on_real_dumps(A):
    """One flipped sign in delta slot 12, one zeroed subtile of delta slot 8, one flipped mask bit, one IDE column of d_allin off by
    2^-10 (fp32 run: bf16 rows cannot hold so small a change), one gradient element moved by twice its tolerance -- each in a COPY of
    what a real run left: the comparators must report each."""
    net = _net(A, "he")
    prec, M = "bf16", 1000
    P = _code(A, prec)
    pts = _inputs(M, 55)
    g_out = _g_out(M, 56)
    out = _forward_train(A, net, prec, pts, "tensor", 0)
    ws, grads = _backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, 0)
    run0 = _read_run(A, prec, M, out, ws, pts[:, 3:6], g_out)
    RB.assert_report("unmodified", _check_stages(A, net, prec, run0, 0, {}, {}, ""))
    R.assert_grads("unmodified", _check_grads(A, prec, run0, grads, {}, ""))
    n_sub, ls = F.geometry(prec, M)
    m, slot = 613, 12
    f = int(run0["deltas"][slot][m].float().abs().argmax())
    assert float(run0["deltas"][slot][m, f]) != 0.0
    # (i) one sign bit in delta slot 12: its own layer and the layer that reads it
    bad = ws.clone()
    bad[R.dump_element_offset(ls, slot, m, f) + 1] ^= 0x80
    run = _read_run(A, prec, M, out, bad, pts[:, 3:6], g_out)
    assert torch.nonzero(run["deltas"][slot] != run0["deltas"][slot]).tolist() == [[m, f]]
    rep = _check_stages(A, net, prec, run, 0, {}, {}, "")
    assert set(RB.failing(rep)) == {"D12", "D11"} and rep["D12"]["where"] == (m, f) and rep["D11"]["where"][0] == m, RB.failing(rep)
    rg = _check_grads(A, prec, run, grads, {}, "")
    assert sorted(k for k, v in rg.items() if not v <= 1.0) in (["w14"], ["b14", "w14"])
    # (ii) one whole subtile of delta slot 8
    bad = ws.clone()
    s = m // 32
    bad[8 * ls + s * 16 * 1024: 8 * ls + (s + 1) * 16 * 1024] = 0
    run = _read_run(A, prec, M, out, bad, pts[:, 3:6], g_out)
    assert not bool((run["s8d"][s * 32: s * 32 + 32] != 0).any()) and torch.equal(run["s8d"][: s * 32], run0["s8d"][: s * 32])
    rep = _check_stages(A, net, prec, run, 0, {}, {}, "")
    failing = set(RB.failing(rep))
    assert {"spec-head", "heads-delta", "bn-order", "D16", "S7"} <= failing, failing
    assert all(rep[k]["where"][0] // 32 == s for k in failing), {k: rep[k]["where"] for k in failing}
    # (iii) one mask bit: the chains of the unmodified run judged with the flipped record
    byte, bit = R.mask_bit(m, f)
    dump_bad = out[2].clone()
    pos = RR.N_SLOTS * ls + slot * n_sub * 1024 + byte
    assert (int(dump_bad[pos]) >> bit) & 1 == 1
    dump_bad[pos] ^= (1 << bit)
    run = _read_run(A, prec, M, (out[0], out[1], dump_bad, out[3], out[4]), ws, pts[:, 3:6], g_out)
    rep = _check_stages(A, net, prec, run, 0, {}, {}, "")
    assert RB.failing(rep) == ["D12", "off-nonzero"] and rep["off-nonzero"]["worst"] == 1.0, RB.failing(rep)
    # (v) one gradient element moved by twice its tolerance
    refs = RB.grad_refs(prec, run0, 2 * A.n_cu)
    moved = dict(grads)
    moved["w15"] = grads["w15"].clone()
    moved["w15"][17, 130] = float(refs["w15"][0][17, 130] + 2.0 * refs["w15"][1][17, 130])
    rg = _check_grads(A, prec, run0, moved, {}, "")
    assert [k for k, v in rg.items() if not v <= 1.0] == ["w15"] and 1.9 < rg["w15"] < 2.1
    # (iv) one IDE column of d_allin off by 2^-10 relative, fp32
    prec = "fp32"
    out = _forward_train(A, net, prec, pts, "tensor", 0)
    ws, grads = _backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, 0)
    run = _read_run(A, prec, M, out, ws, pts[:, 3:6], g_out)
    RB.assert_report("unmodified fp32", _check_stages(A, net, prec, run, 0, {}, {}, ""))
    run["d_allin"] = run["d_allin"].clone()
    run["d_allin"][:, 128 + 7] *= 1.0 + 2.0 ** -10
    rep = _check_stages(A, net, prec, run, 0, {}, {}, "")
    assert "heads-delta" in RB.failing(rep) and set(RB.failing(rep)) <= {"heads-delta", "dallin"}, RB.failing(rep)
