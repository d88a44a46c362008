"""The workspaces of the training backward's host side (nerf_amd/csrc/bwd_kernels.hip: the weight-gradient products of the proposal and
MipNeRF networks, the Ref-NeRF parameter backward) as the CALLER sees them: nerf_amd_proposal_weight_grads, nerf_amd_mip_weight_grads
and nerf_amd_ref_backward through ctypes on storage this test owns, with exactly the bytes the size query asks for.

Per (network, precision, dump format, M):
  1. the 4096 canary bytes behind `need` keep their pattern: the carving stays inside what the size query promised;
  2. the workspace base 0, 4 and 252 bytes behind a 256-aligned address, `need` bytes from there: every gradient bit-identical (the
     + 256 / + 512 slack of the size is what pays for aligning the base);
  3. workspace and outputs pre-filled with 0x00 and with 0xFF bytes: bit-identical and finite (Ref-NeRF at M = 1 and 257: asserted by
     test_gpu_ref_backward_layers.test_nothing_is_read_before_it_is_written, which is called, not repeated).
M = 1: every batch's workgroup count is clipped by the subtile count; 257: a second tile; 16417 = 16384 + 33: at least 513 subtiles on
either tile size, so that on 256 compute units even a light single-product batch gets its full 2 x 256 workgroups.
On 256 compute units the size queries must also equal tests/golden/backward_workspace_bytes.json on the GPU."""
import pytest
import torch

import backward_ref as R
import test_gpu_backward_layers as PM
import test_gpu_ref_backward_layers as RF
from test_abi_and_host import test_backward_workspace_sizes_are_the_documented_closed_forms as _sizes_test
from test_gpu_ref_forward_layers import _code, _forward_train, _inputs as _ref_inputs

pytestmark = pytest.mark.gpu

SIZES = (1, 257, 16417)
PM_MODES = (("fp32", "bf16"), ("bf16", "bf16"), ("bf16", "fp8"))        # (arithmetic, dump format of the hidden slots)
TAIL = 4096
OFFSETS = (0, 4, 252)


@pytest.fixture(scope="module")
def A():
    """what the A fixtures of the two layer-test modules hold, so that their helpers serve here"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return make_namespace()


def make_namespace():
    import ctypes
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


def _canary():
    return (torch.arange(TAIL, device="cuda") % 251 + 1).to(torch.uint8)


def workspace(need, off, fill):
    """-> (`need` bytes `off` bytes behind a 256-aligned address, pre-filled with `fill`; the TAIL canary bytes behind them)"""
    buf = torch.full((need + TAIL + 512,), fill, dtype=torch.uint8, device="cuda")
    a = (-buf.data_ptr()) % 256 + off
    buf[a + need: a + need + TAIL] = _canary()
    ws = buf[a: a + need]
    assert ws.data_ptr() % 256 == off
    return ws, buf[a + need: a + need + TAIL]


def prepare(A, name, prec, fmt, M):
    """forward and dgrad chain of one case -> (need, call(ws, fill) -> {name: gradient tensor}); outputs pre-filled like the workspace"""
    ops, lib = A.ops, A.lib
    if name == "ref":
        net = RF._net(A, "he")
        pts = _ref_inputs(M, 11 + M % 997)
        out = _forward_train(A, net, prec, pts, "none", 0)
        g_out = RF._g_out(M, 9 + M % 997)
        need = lib.nerf_amd_ref_backward_workspace_bytes(_code(A, prec), M)
        return need, lambda ws, fill: RF._backward(A, net, prec, out[2], out[3], pts[:, 3:6], g_out, 0, fill, ws)[1]
    net = PM._net(A, name, "he")
    _, T = PM._codes(A, prec, fmt)
    pts, g = PM._inputs(name, M, 11 + M % 997)
    out, dump = PM._forward(A, net, prec, fmt, pts)
    delta = PM._chain(A, net, prec, fmt, g, out, dump)
    need = lib.nerf_amd_weight_grads_workspace_bytes(net.id, T, M)
    shapes = [tuple(w.shape) for w in net.ws]

    def call(ws, fill):
        gw = [RF._filled(4 * s[0] * s[1], fill).view(torch.float32).view(s) for s in shapes]
        gb = [RF._filled(4 * s[0], fill).view(torch.float32) for s in shapes]
        if name == "prop":
            rc = lib.nerf_amd_proposal_weight_grads(T, M, ops._ptr(dump), ops._ptr(delta), ops._ptr_array(gw), ops._ptr_array(gb), ops._ptr(ws), ops._stream())
        else:
            rc = lib.nerf_amd_mip_weight_grads(T, M, ops._ptr(dump), ops._ptr(delta), ops._ptr_array(net.ws), ops._ptr_array(net.bs), ops._ptr_array(gw),
                                               ops._ptr_array(gb), ops._ptr(ws), ops._stream())
        ops.check(rc, "nerf_amd_%s_weight_grads" % ("proposal" if name == "prop" else "mip"))
        return R.named_grads(gw, gb)
    return need, call


def _check_case(A, name, prec, fmt, M, prefill_pinned_elsewhere=False):
    need, call = prepare(A, name, prec, fmt, M)
    assert need > 0
    runs = [(off, 0x00) for off in OFFSETS] + ([] if prefill_pinned_elsewhere else [(0, 0xFF)])
    first = None
    for off, fill in runs:
        ws, tail = workspace(need, off, fill)
        grads = call(ws, fill)
        torch.cuda.synchronize()
        what = (name, prec, fmt, M, "base + %d" % off, "0x%02X" % fill)
        assert torch.equal(tail, _canary()), ("bytes behind the queried size were written",) + what
        assert all(bool(torch.isfinite(g).all()) for g in grads.values()), what
        bits = {k: g.view(torch.int32).clone() for k, g in grads.items()}
        if first is None:
            first = bits
        for k in first:
            assert torch.equal(first[k], bits[k]), (k,) + what
        del ws, tail, grads


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("prec,fmt", PM_MODES)
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_products_stay_inside_the_queried_workspace_at_any_base_alignment(A, name, prec, fmt, M):
    _check_case(A, name, prec, fmt, M)


_PINNED = {}


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_ref_backward_stays_inside_the_queried_workspace_at_any_base_alignment(A, prec, M):
    pinned = M in (1, 257)                                      # among the sizes of test_nothing_is_read_before_it_is_written
    if pinned and prec not in _PINNED:
        RF.test_nothing_is_read_before_it_is_written(A, prec)
        _PINNED[prec] = True
    _check_case(A, "ref", prec, "bf16", M, prefill_pinned_elsewhere=pinned)


def test_size_queries_equal_the_recorded_table_on_the_gpu(A):
    """(the host test reads the device's compute-unit count when there is a GPU and compares with the table at 256)"""
    if A.n_cu != 256:
        pytest.skip("the recorded table holds for 256 compute units (this device: %d)" % A.n_cu)
    _sizes_test()
