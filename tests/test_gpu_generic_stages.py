"""The kernels of the layer-by-layer route (nerf_amd/generic_path.py) one stage at a time against the fp64 specifications and element-wise
bounds of tests/generic_ref.py (checked on the CPU by tests/test_generic_ref_host.py): the element-wise stages of generic_ref_kernels.hip /
generic_kernels.hip on contiguous tensors AND on the views the route passes, at sample counts on both sides of a 256-thread block;
nerf_amd_gemm in every operand form (offset bases, vectorisable and non-vectorisable strides, both memory orders, column-range masks and
outputs, the re-layout switch, the split contraction); nerf_amd_rows_to_bf16 on crafted bit patterns; nerf_amd_rows_gemm at every stage
count of its rings.  Every gate is max(err / tol) <= 1 over every element."""
import pytest
import torch

import generic_ref as R
from conftest import gate, max_abs
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
SENT = -7.25
BD = 128                                     # the bottle-neck width in front of the directional inputs (cat2[:, Bd:Din])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


@pytest.fixture(scope="module")
def ops():
    from nerf_amd import ops
    return ops


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int16)


def guarded(M, cols, fill=SENT, dtype=torch.float32):
    """-> (whole, rows): rows = M rows of a sentinel-filled (M + 4, cols) device buffer, two guard rows on either side"""
    whole = torch.full((M + 4, cols), fill, dtype=dtype, device="cuda")
    return whole, whole[2:M + 2]


def put(M, cols, c0, src, fill=SENT):
    """src (M, n) on the device as columns [c0, c0 + n) of a sentinel-filled guarded (M, cols) buffer -> (whole, view)"""
    whole, rows = guarded(M, cols, fill)
    rows[:, c0:c0 + src.shape[1]] = src.cuda()
    return whole, rows[:, c0:c0 + src.shape[1]]


def assert_untouched(whole, before, written):
    """everything of `whole` outside the boolean mask `written` (same shape) is bit-unchanged"""
    assert torch.equal(bits(whole)[~written], bits(before)[~written]), "storage outside the documented output columns was written"


def table(deg):
    return O.ide_tables(deg)[1].contiguous().cuda()


# ------------------------------------------------------------------------------------------------ the directional stage
@pytest.mark.parametrize("M", R.MS)
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_ref_dir_inputs(ops, deg, M):
    """ref_dir_inputs<deg> on contiguous tensors and on the route's views (heads = columns 2:13 of a 16-wide buffer, dirs = rays[:, 3:],
    out = cat2[:, Bd:Din]): normal, n.d and every IDE term inside their bounds, the views bit-identical, nothing else written"""
    h, d, _, _, _, _ = R.dir_inputs(M, deg)
    T = R.T_of(deg)
    out_c = torch.full((M, 2 * T + 1), SENT, device="cuda")
    n_c = ops.ref_dir_inputs(h.cuda(), d.cuda(), deg, table(deg), out_c)
    rep = R.dir_forward_check(h, d, deg, out_c, n_c)
    for k, r in rep.items():
        gate("ref_dir_inputs<%d> M %d %s: max(err / tol) at %s" % (deg, M, k, r["where"]), r["worst"], 1.0)
    _, hv = put(M, 16, 2, h)
    _, dv = put(M, 6, 3, d)
    Din = BD + 2 * T + 1
    whole, cat2 = guarded(M, Din + 8)
    before = whole.clone()
    n_v = ops.ref_dir_inputs(hv, dv, deg, table(deg), cat2[:, BD:Din])
    written = torch.zeros_like(whole, dtype=torch.bool)
    written[2:M + 2, BD:Din] = True
    assert_untouched(whole, before, written)
    assert torch.equal(bits(cat2[:, BD:Din]), bits(out_c)) and torch.equal(bits(n_v), bits(n_c))
    assert not bool((bits(out_c) == bits(torch.full_like(out_c, SENT))).any())           # every output column was written


@pytest.mark.parametrize("M", R.MS)
@pytest.mark.parametrize("deg", [1, 2, 3, 4, 5])
def test_ref_dir_inputs_backward(ops, deg, M):
    """ref_dir_inputs_backward<deg>: columns 0-2 and 9 of d_heads against fp64 autograd, on contiguous tensors and on the route's views
    (d_out = d_all[:, Bd:], g_normal = g7[:, 4:7], d_heads = the first 11 columns of an (M, 11 + Bd) buffer); every other column untouched"""
    h, d, do, gn, _, _ = R.dir_inputs(M, deg)
    T = R.T_of(deg)
    dh_c = torch.full((M, 11), SENT, device="cuda")
    ops.ref_dir_inputs_backward(h.cuda(), d.cuda(), deg, table(deg), do.cuda(), gn.cuda(), dh_c)
    r = R.compare(dh_c[:, [0, 1, 2, 9]], *R.dir_backward_spec(h, d, deg, do, gn))
    gate("ref_dir_inputs_backward<%d> M %d: max(err / tol) at %s" % (deg, M, r["where"]), r["worst"], 1.0)
    cols = torch.tensor([c in (0, 1, 2, 9) for c in range(11)], device="cuda")
    sent = bits(dh_c) == bits(torch.full_like(dh_c, SENT))
    assert bool(sent[:, ~cols].all()) and not bool(sent[:, cols].any())                  # exactly columns 0-2 and 9, in every row
    _, hv = put(M, 16, 2, h)
    _, dv = put(M, 6, 3, d)
    _, dov = put(M, BD + 2 * T + 1, BD, do)
    _, gnv = put(M, 7, 4, gn)
    whole, dhb = guarded(M, 11 + BD)
    before = whole.clone()
    ops.ref_dir_inputs_backward(hv, dv, deg, table(deg), dov, gnv, dhb)
    written = torch.zeros_like(whole, dtype=torch.bool)
    written[2:M + 2, [0, 1, 2, 9]] = True
    assert_untouched(whole, before, written)
    assert torch.equal(bits(dhb[:, :11]), bits(dh_c))
    # ref_combine_backward into the same buffer: the 11 head columns are each written exactly once by the two kernels together
    hc, sc, gc = R.combine_inputs(M, False)
    ops.ref_combine_backward(gc.cuda(), hc.cuda(), sc.cuda(), 0, dhb)
    assert torch.equal(bits(dhb[:, [0, 1, 2, 9]]), bits(dh_c[:, [0, 1, 2, 9]]))
    assert not bool((bits(dhb[:, :11]) == bits(torch.full_like(dhb[:, :11], SENT))).any())
    assert torch.equal(bits(whole[:, 11:]), bits(before[:, 11:]))


# ------------------------------------------------------------------------------------------------ the colour combination
@pytest.mark.parametrize("M", R.MS)
@pytest.mark.parametrize("use_srgb", [False, True])
def test_ref_combine_and_backward(ops, use_srgb, M):
    """ref_combine and ref_combine_backward (columns 3-8 and 10 of d_heads, and d_spec), contiguous and on views (heads = columns 2:13 of
    16, spec = columns 1:4 of 5, g_rgbo = g7[:, :4], d_heads in an (M, 11 + Bd) buffer).  Together with ref_dir_inputs_backward's
    columns 0-2 and 9 each of the 11 head columns is written exactly once."""
    h, s, g = R.combine_inputs(M, use_srgb)
    flags = ops.REF_SRGB if use_srgb else 0
    tag = "srgb" if use_srgb else "linear"
    rgbo_c = ops.ref_combine(h.cuda(), s.cuda(), flags)
    r = R.compare(rgbo_c, *R.combine_spec(h, s, use_srgb))
    gate("ref_combine %s M %d: max(err / tol) at %s" % (tag, M, r["where"]), r["worst"], 1.0)
    dh_c = torch.full((M, 11), SENT, device="cuda")
    dsp_c = ops.ref_combine_backward(g.cuda(), h.cuda(), s.cuda(), flags, dh_c)
    want_spec, want_heads = R.combine_backward_spec(g, h, s, use_srgb)
    r1, r2 = R.compare(dsp_c, *want_spec), R.compare(dh_c[:, [3, 4, 5, 6, 7, 8, 10]], *want_heads)
    gate("ref_combine_backward %s M %d d_spec: max(err / tol) at %s" % (tag, M, r1["where"]), r1["worst"], 1.0)
    gate("ref_combine_backward %s M %d d_heads: max(err / tol) at %s" % (tag, M, r2["where"]), r2["worst"], 1.0)
    mine = torch.tensor([c in (3, 4, 5, 6, 7, 8, 10) for c in range(11)], device="cuda")
    sent = bits(dh_c) == bits(torch.full_like(dh_c, SENT))
    assert bool(sent[:, ~mine].all()) and not bool(sent[:, mine].any())
    _, hv = put(M, 16, 2, h)
    _, sv = put(M, 5, 1, s)
    _, gv = put(M, 7, 0, g)
    rgbo_v = ops.ref_combine(hv, sv, flags)
    whole, dhb = guarded(M, 11 + BD)
    before = whole.clone()
    dsp_v = ops.ref_combine_backward(gv, hv, sv, flags, dhb)
    written = torch.zeros_like(whole, dtype=torch.bool)
    written[2:M + 2, [3, 4, 5, 6, 7, 8, 10]] = True
    assert_untouched(whole, before, written)
    assert torch.equal(bits(rgbo_v), bits(rgbo_c)) and torch.equal(bits(dsp_v), bits(dsp_c)) and torch.equal(bits(dhb[:, :11]), bits(dh_c))


# ------------------------------------------------------------------------------------------------ PE adjoint, add_rows, sigmoid adjoint, contraction
@pytest.mark.parametrize("cat_origin", [True, False])
@pytest.mark.parametrize("L", [4, 10, 12, 16])
def test_positional_encoding_backward(ops, L, cat_origin):
    """pe_backward at M on both sides of a block (85 / 86 samples = 255 / 258 threads), d_enc contiguous and as the first E columns of an
    (M, E + W) buffer, x contiguous and with row stride 6; the reference's sine arguments 2^f x32 are exact"""
    worst = 0.0
    for M in R.MS + (85, 86):
        x, de = R.pe_inputs(M, L, cat_origin)
        got = ops.positional_encoding_backward(de.cuda(), x.cuda(), L, cat_origin)
        r = R.compare(got, *R.pe_backward_spec(de, x, L, cat_origin))
        worst = max(worst, r["worst"])
        assert r["worst"] <= 1.0, (M, r)
        _, dev_ = put(M, de.shape[1] + 24, 0, de)
        _, xv = put(M, 6, 0, x)
        assert torch.equal(bits(ops.positional_encoding_backward(dev_, xv, L, cat_origin)), bits(got)), M
    gate("positional_encoding_backward L %d cat_origin %d: max(err / tol) over M" % (L, cat_origin), worst, 1.0)


@pytest.mark.parametrize("cols", [1, 3, 128])
def test_add_rows_is_the_fp32_sum(ops, cols):
    for M in R.MS:
        g = torch.Generator().manual_seed(cols + M)
        a, b = torch.randn(M, cols, generator=g), torch.randn(M, cols, generator=g) * 3
        whole, dst = put(M, cols + 5, 2, a)
        _, src = put(M, cols + 2, 1, b)
        before = whole.clone()
        ops.add_rows_(dst, src)
        written = torch.zeros_like(whole, dtype=torch.bool)
        written[2:M + 2, 2:2 + cols] = True
        assert_untouched(whole, before, written)
        assert torch.equal(bits(dst), bits((a + b).cuda())) and max_abs(dst.cpu(), a + b) == 0.0, (M, cols)
        c = a.cuda()
        assert torch.equal(bits(ops.add_rows_(c, b.cuda())), bits((a + b).cuda()))


def test_sigmoid_backward(ops):
    """g y (1 - y) on gr[:, :3] and out[:, :3] of 4-wide buffers within 3 u relative (two products and a difference); y = 0 and y = 1 give 0"""
    worst = 0.0
    for M in R.MS:
        g = torch.Generator().manual_seed(M)
        gr, y = torch.randn(M, 3, generator=g), torch.sigmoid(torch.randn(M, 3, generator=g) * 3)
        y[0, 0] = 0.0
        y[M // 2, 1] = 1.0
        y[M - 1, 2] = 0.0
        ref = gr.double() * y.double() * (1 - y.double())
        _, gv = put(M, 4, 0, gr)
        _, yv = put(M, 4, 0, y)
        got = ops.sigmoid_backward(gv, yv)
        r = R.compare(got, ref, 3 * R.U * ref.abs() + R.TINY * (ref != 0))
        worst = max(worst, r["worst"])
        assert r["worst"] <= 1.0, (M, r)
        assert torch.equal(bits(ops.sigmoid_backward(gr.cuda(), y.cuda())), bits(got))
    gate("sigmoid_backward: max(err / (3 u |ref|)) over M", worst, 1.0)


def test_contract_positions(ops):
    """forward and pull-back against oracle.contract and its fp64 autograd: radii 0, 1, nextafter(1, 2), 1e6 among the rows, contiguous and
    with row stride 6"""
    wf = wb = 0.0
    for M in R.MS:
        x, g = R.contract_inputs(M)
        got, pb = ops.contract_positions(x.cuda()), ops.contract_positions(x.cuda(), grad=g.cuda())
        rf, rb = R.compare(got, *R.contract_spec(x)), R.compare(pb, *R.contract_spec(x, g))
        assert rf["worst"] <= 1.0 and rb["worst"] <= 1.0, (M, rf, rb)
        wf, wb = max(wf, rf["worst"]), max(wb, rb["worst"])
        _, xv = put(M, 6, 0, x)
        _, gv = put(M, 6, 3, g)
        assert torch.equal(bits(ops.contract_positions(xv)), bits(got)) and torch.equal(bits(ops.contract_positions(xv, grad=gv)), bits(pb))
    gate("contract_positions forward: max(err / tol) over M", wf, 1.0)
    gate("contract_positions pull-back: max(err / tol) over M", wb, 1.0)


# ------------------------------------------------------------------------------------------------ nerf_amd_gemm: operand forms
PRECS = ["fp32", "bf16"]


def code(ops, prec):
    return ops.F32 if prec == "fp32" else ops.BF16


def operand(rows, cols, off, ld, gen, transposed):
    """a (rows, cols) fp32 device view at element offset `off` of a buffer of finite junk: row stride ld, or (transposed) the
    transpose of a (cols, rows) matrix with row stride ld.  -> the view (its .cpu() is what the reference reads)"""
    r, c = (cols, rows) if transposed else (rows, cols)
    assert ld >= c
    store = torch.randn(off + r * ld + 8, generator=gen).cuda()
    v = store[off:off + r * ld].view(r, ld)[:, :c]
    return v.t() if transposed else v


@pytest.mark.parametrize("P", [1, 3, 4, 5, 31, 32, 33, 63, 65])
@pytest.mark.parametrize("prec", PRECS)
def test_gemm_offset_bases_and_strides(ops, prec, P):
    """A and B at element offsets 1-4 of a larger buffer (offset 4 = a 16-byte aligned base), row strides = 0 and != 0 (mod 4), each
    operand in the contraction-contiguous and in the output-contiguous order: every combination of the 16-byte / scalar load choice
    (aligned16(...) && stride % 4 == 0) and of the n_valid < 4 tails, with bias and ReLU"""
    M, N = 37, 29
    gen = torch.Generator().manual_seed(1000 + P)
    bias = torch.randn(N, generator=gen)
    worst = 0.0
    for off in (1, 2, 3, 4):
        for pad in (4, 5):
            for ta in (False, True):
                for tb in (False, True):
                    lda = ((M if ta else P) + 3) // 4 * 4 + pad
                    ldb = ((P if tb else N) + 3) // 4 * 4 + pad
                    a, b = operand(M, P, off, lda, gen, ta), operand(P, N, off, ldb, gen, tb)
                    got = ops.gemm(code(ops, prec), a, b, bias=bias.cuda(), act=1)
                    r = R.compare(got, *R.gemm_spec(a, b, prec, bias, 1))
                    assert r["worst"] <= 1.0, (off, pad, ta, tb, r)
                    worst = max(worst, r["worst"])
    gate("gemm %s P %d offsets x strides x orders: max(err / tol)" % (prec, P), worst, 1.0)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_route_views(ops, prec):
    """the operand views of the route: w20[:, :Din] / w20[:, Din:] with Din odd, g7[:, 3:4] (an (M, 1) view with row stride 7) times
    rt.weight[1:2, :] (a row of a matrix) under a mask, mask = q[:, Din:] (ldm != N) holding -0.0, +0.0, a denormal and a NaN -- the
    kernel's rule is !(mask > 0) -> 0 --, out as a column range with sentinel neighbours"""
    gen = torch.Generator().manual_seed(7)
    M, Din, W, N0 = 257, 191, 72, 130
    delta = torch.randn(M, N0, generator=gen)
    w20 = (torch.randn(N0, Din + W, generator=gen) * 0.1).cuda()
    q = torch.relu(torch.randn(M, Din + W, generator=gen))
    q[0, Din], q[1, Din + 1], q[2, Din + 2], q[3, Din + 3] = -0.0, 0.0, 1e-42, float("nan")
    q[255, Din + W - 1], q[256, Din] = float("nan"), 1e-45
    qd = q.cuda()
    for name, b, mask in (("w20[:, :Din]", w20[:, :Din], None), ("w20[:, Din:] masked", w20[:, Din:], qd[:, Din:])):
        whole, rows = guarded(M, b.shape[1] + 7)
        before = whole.clone()
        out = rows[:, 3:3 + b.shape[1]]
        ops.gemm(code(ops, prec), delta.cuda(), b, out=out, mask=mask)
        written = torch.zeros_like(whole, dtype=torch.bool)
        written[2:M + 2, 3:3 + b.shape[1]] = True
        assert_untouched(whole, before, written)
        r = R.compare(out, *R.gemm_spec(delta, b, prec, mask=mask))
        gate("gemm %s %s: max(err / tol) at %s" % (prec, name, r["where"]), r["worst"], 1.0)
        if mask is not None:
            m = mask.cpu()
            closed = ~(m > 0)
            assert bool(closed[0, 0] and closed[1, 1] and closed[3, 3] and closed[255, W - 1]) and not bool(closed[2, 2] or closed[256, 0])
            assert float(out.cpu()[closed].abs().max()) == 0.0 and bool((out.cpu()[~closed] != 0).all())
    g7 = torch.randn(M, 7, generator=gen).cuda()
    rtw = torch.randn(2, N0, generator=gen).cuda()
    gm = torch.relu(torch.randn(M, N0 + 3, generator=gen)).cuda()[:, 1:1 + N0]
    got = ops.gemm(code(ops, prec), g7[:, 3:4], rtw[1:2, :], mask=gm)
    r = R.compare(got, *R.gemm_spec(g7[:, 3:4], rtw[1:2, :], prec, mask=gm))
    gate("gemm %s g7[:, 3:4] x rt.weight[1:2, :] masked: max(err / tol)" % prec, r["worst"], 1.0)
    one = ops.gemm(code(ops, prec), rtw[1:2, :], delta.cuda().t())                      # (1, P) row of a matrix as A
    r = R.compare(one, *R.gemm_spec(rtw[1:2, :], delta.t(), prec))
    gate("gemm %s rt.weight[1:2, :] as A: max(err / tol)" % prec, r["worst"], 1.0)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_tile_edges_and_grids(ops, prec):
    """M, N in {127, 128, 129}; grids of 1 x 9, 9 x 1 and 3 x 5 tiles (tiles_m < tiles_n, 15 workgroups: not a multiple of 8)"""
    gen = torch.Generator().manual_seed(11)
    shapes = [(M, N) for M in (127, 128, 129) for N in (127, 128, 129)] + [(100, 9 * 128 - 5), (9 * 128 - 5, 100), (3 * 128 - 1, 5 * 128 - 3)]
    worst, P = 0.0, 33
    for M, N in shapes:
        a, w, bias = torch.randn(M, P, generator=gen), torch.randn(N, P, generator=gen), torch.randn(N, generator=gen)
        got = ops.gemm(code(ops, prec), a.cuda(), w.cuda().t(), bias=bias.cuda())
        r = R.compare(got, *R.gemm_spec(a, w.t(), prec, bias))
        assert r["worst"] <= 1.0, (M, N, r)
        worst = max(worst, r["worst"])
    gate("gemm %s tile edges and grid shapes: max(err / tol)" % prec, worst, 1.0)


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_relayout_switch(ops, prec):
    """the input-gradient form dy W at M = 4095 and 4096, the two sides of the re-layout of W in ops.gemm: the matrix cores add the
    products of a stage in the same order whichever memory order W was staged from, so rows 0 .. 4094 are bit-equal"""
    gen = torch.Generator().manual_seed(13)
    dy, w = torch.randn(4096, 40, generator=gen), torch.randn(40, 72, generator=gen)
    mask = torch.relu(torch.randn(4096, 72, generator=gen))
    big = ops.gemm(code(ops, prec), dy.cuda(), w.cuda(), mask=mask.cuda())
    small = ops.gemm(code(ops, prec), dy[:4095].cuda(), w.cuda(), mask=mask[:4095].cuda())
    r = R.compare(big, *R.gemm_spec(dy, w, prec, mask=mask))
    gate("gemm %s input gradient M 4096 (re-laid out): max(err / tol)" % prec, r["worst"], 1.0)
    r = R.compare(small, *R.gemm_spec(dy[:4095], w, prec, mask=mask[:4095]))
    gate("gemm %s input gradient M 4095: max(err / tol)" % prec, r["worst"], 1.0)
    assert torch.equal(bits(big[:4095]), bits(small))


def split_count(M, N, P, cu):
    """generic_kernels.hip split_count / gk_gemm: -> (slices, contraction elements per slice)"""
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if P < 4096 or tiles >= 512:
        return 1, max(P, 1)
    s = min((4 * cu + tiles - 1) // tiles, (P + 127) // 128, 1024)
    s = max(s, 1)
    return s, ((P + s - 1) // s + 31) // 32 * 32


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_split_contraction(ops, prec):
    """the split path (workspace > 0) and its reduce kernel's epilogue with bias, every activation and a mask, against the UNSPLIT
    specification; run twice, bit-equal.  The third shape's contraction length is chosen from the device's CU count so that the chunk,
    rounded up to 32, leaves the last slices EMPTY (asserted)."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    M3 = N3 = 130
    s_cu = (4 * cu + 3) // 4
    shapes = [(40, 24, 4096), (40, 24, 4100), (M3, N3, 128 * s_cu + 32)]
    S, chunk = split_count(*shapes[2], cu)
    assert S == s_cu and (S - 1) * chunk >= shapes[2][2], "the empty-slice case was not reached: %d slices of %d over %d" % (S, chunk, shapes[2][2])
    gen = torch.Generator().manual_seed(17)
    for M, N, P in shapes:
        assert ops.lib.nerf_amd_gemm_workspace_bytes(M, N, P) == split_count(M, N, P, cu)[0] * M * N * 4 > 0
        a, b = torch.randn(P, M, generator=gen), torch.randn(P, N, generator=gen)      # the weight-gradient form dy^T x
        bias, mask = torch.randn(N, generator=gen), torch.relu(torch.randn(M, N + 3, generator=gen))
        mask[0, 1] = float("nan")
        ad, bd, maskd = a.cuda(), b.cuda(), mask.cuda()[:, 1:1 + N]
        q = (lambda t: t.bfloat16().double()) if prec == "bf16" else (lambda t: t.double())
        pre = (q(a).t() @ q(b), q(a).abs().t() @ q(b).abs())
        for act in (0, 1, 2):
            got = ops.gemm(code(ops, prec), ad.t(), bd, bias=bias.cuda(), act=act, mask=maskd)
            again = ops.gemm(code(ops, prec), ad.t(), bd, bias=bias.cuda(), act=act, mask=maskd)
            assert torch.equal(bits(got), bits(again))
            r = R.compare(got, *R.gemm_spec(a.t(), b, prec, bias, act, maskd, pre=pre))
            gate("gemm %s split %d x %d x %d act %d: max(err / tol) at %s" % (prec, M, N, P, act, r["where"]), r["worst"], 1.0)
            assert float(got[0, 0]) == 0.0                                               # the NaN of the mask closes its element


@pytest.mark.parametrize("prec", PRECS)
def test_gemm_empty_contraction_is_act_of_bias(ops, prec):
    bias = torch.tensor([-2.0, 0.0, 0.5, 3.0, -0.0])
    for act, f in ((0, lambda t: t), (1, torch.relu), (2, torch.sigmoid)):
        got = ops.gemm(code(ops, prec), torch.empty((130, 0), device="cuda"), torch.empty((0, 5), device="cuda"), bias=bias.cuda(), act=act)
        ref = f(bias.double()).expand(130, 5)
        assert R.compare(got, ref, R.SIG_U * R.U * ref.abs() if act == 2 else torch.zeros_like(ref))["worst"] <= 1.0, act


# ------------------------------------------------------------------------------------------------ rows_to_bf16, rows_gemm
def test_rows_to_bf16_bit_patterns(ops):
    """RNE against tensor.bfloat16() on crafted patterns: exact ties with even and odd kept mantissa, one ulp either side of a tie, the
    largest finite fp32 (-> Inf), +-Inf, NaNs, +-0, denormals; rows > rows_src and fill > cols are zero; a destination column offset
    with sentinels around the written range"""
    pats = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF, 0x3F7F8000, 0x3FFF8000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
            0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FC12345, 0x00000000, 0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF,
            0x007F8000, 0x00800000, 0x33800000, 0x477FE000]
    pats = pats + [p | 0x80000000 for p in pats]
    R_, C = 5, len(pats) + 3                                                             # an odd width: fill rounds it up
    src = torch.tensor(pats + [0x3F800000] * 3, dtype=torch.int64).to(torch.int32).view(torch.float32).repeat(R_, 1).contiguous()
    src[1:, :] = src[1:, :].flip(1)
    want = src.bfloat16()
    rows, col0, fill = R_ + 3, 8, C + 6
    whole, dst = guarded(rows + 1, col0 + fill + 5, fill=7.0, dtype=torch.bfloat16)
    before = whole.clone()
    ops.rows_to_bf16(src.cuda(), dst, col0, fill, rows)
    written = torch.zeros_like(whole, dtype=torch.bool)
    written[2:rows + 2, col0:col0 + fill] = True
    assert_untouched(whole, before, written)
    got = dst[:R_, col0:col0 + C].cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    mism = (bits(got) != bits(want)) & ~nan
    assert not bool(mism.any()), "first mismatch: fp32 pattern %#010x -> %#06x, torch %#06x" % (
        int(bits(src)[mism][0]) & 0xffffffff, int(bits(got)[mism][0]) & 0xffff, int(bits(want)[mism][0]) & 0xffff)
    assert bool(torch.isinf(got[0, 8])) and float(got[0, 0]) == 1.0 and float(got[0, 1]) == 1.015625       # 0x7F7FFFFF -> Inf; ties to even
    zeros = bits(dst[:rows, col0:col0 + fill].cpu())
    assert int(zeros[R_:].abs().max()) == 0 and int(zeros[:, C:].abs().max()) == 0       # the extra rows and the padding columns: +0


ROWS_K = (31, 32, 33, 64, 65, 96, 97, 128)


def _rows_case(ops, M, N, K, act, dt, c0, gen):
    """existing comparator and limits of test_layer_products_on_bf16_rows: fp64 on the rounded operands, error relative to 1 + |want|;
    X = a column range whose padding columns (K .. roundup(K, 8)) and neighbours hold finite junk"""
    x32, w, b = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, torch.randn(N, generator=gen)
    buf = torch.full((M, c0 + ops._pad(K, 8) + 8), 7.0, dtype=torch.bfloat16, device="cuda")
    ops.rows_to_bf16(x32.cuda(), buf, c0, K)                                              # fill = K: the padding columns keep the junk
    layer = ops.PackedLinear(w.cuda(), b.cuda())
    got = ops.rows_gemm(buf[:, c0:c0 + K], layer, act, out_dtype=dt)
    assert got.shape == (M, N) and got.dtype == dt
    want = x32.bfloat16().double() @ w.bfloat16().double().t() + b.double()
    want = want.clamp(min=0) if act == 1 else (torch.sigmoid(want) if act == 2 else want)
    return float(((got.float().cpu().double() - want).abs() / (1.0 + want.abs())).max())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rows_gemm_stage_counts_128x256(ops, dt):
    """the 128 x 256 configuration (32-wide stages on a 3-slot ring): K giving 1 .. 4 stages, M in {127, 128, 129} at a full (N = 256) and
    a ragged (N = 320) feature tile"""
    gen = torch.Generator().manual_seed(19)
    lim = 1e-5 if dt == torch.float32 else 4e-3
    worst = 0.0
    for K in ROWS_K:
        for M, N in ((129, 256), (127, 320)):
            worst = max(worst, _rows_case(ops, M, N, K, 1, dt, 8 * (K % 3), gen))
    for M in (127, 128, 129):
        for N in (256, 320):
            worst = max(worst, _rows_case(ops, M, N, 97, 0, dt, 0, gen))
    gate("rows_gemm 128 x 256 tiles, K %s -> %s: vs fp64 on the rounded operands" % (ROWS_K, str(dt).split(".")[1]), worst, lim)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_rows_gemm_stage_counts_256x256(ops, dt):
    """the 256 x 256 configuration (64-wide stages on a 2-slot ring): M in {255, 256, 257}, N in {512, 768}, K in {64, 65, 128} = 1 .. 2 stages"""
    gen = torch.Generator().manual_seed(23)
    lim = 1e-5 if dt == torch.float32 else 4e-3
    worst = 0.0
    for M in (255, 256, 257):
        for N in (512, 768):
            for K in (64, 65, 128):
                worst = max(worst, _rows_case(ops, M, N, K, 1 if K != 65 else 2, dt, 8 * (M % 2), gen))
    gate("rows_gemm 256 x 256 tiles -> %s: vs fp64 on the rounded operands" % str(dt).split(".")[1], worst, lim)
