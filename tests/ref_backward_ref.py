"""The Ref-NeRF counterpart of tests/backward_ref.py: fp64 references with worst-case element-wise bounds for every stage of the Ref-NeRF
parameter backward (bwd_ref_backward) and of the density-gradient chains (bwd_density_grad), nerf_amd/csrc/bwd_kernels.hip, each stage
against ITS OWN INPUTS as the kernels left them.  Plain helper module (no fixtures), built on backward_ref.py (layout, chain / product
comparators and bounds) and ref_forward_ref.py (slot 8, the running error analysis of the element-wise expressions):
tests/test_gpu_ref_backward_layers.py feeds it the activation dump, its mask records, aux, dirs, g_out and the workspace the kernels
wrote; tests/test_ref_backward_ref_host.py feeds it a torch fp64 forward (composition == torch.autograd), an honest fp32 / bf16
emulation (every ratio <= 1) and nine planted faults.

THE WORKSPACE (bwd_ref_backward's Carver; base aligned to 256): the delta dump, REF_DUMP_SLOTS = 17 slots of the activation dump's layer
stride, at offset 0; d_allin (M, 192) at align256(17 stride) -- fp32 rows, or bf16 rows of the SAME element layout in bf16 precision
(RowsOutT<true>); the products' partial sums behind align256(M 192 4).  Delta slot L = delta of the layer whose activations sit in
activation slot L; delta slot 8: K groups 0..7 delta of the bottle-neck, K group 8 the 11 head rows (kernel order: normal 0-2, roughness 3,
diffuse 4-6, density 7, tint 8-10), K group 9 the spec head (features 0..2); K groups 10..15 are never written and never read.
bwd_density_grad's workspace: d_enc (M, 64) fp32 at offset 0.

STAGES AND BOUNDS (u = 2^-24; the library is built with -ffp-contract=off and without fast-math: every operator of the source is one
rounded fp32 operation):
  a  spec head   v_c = ((g_c f'_c) sig(tint_c)) (sp_c (1 - sp_c)):  running error analysis (ref_forward_ref's _mul / _add / _sigmoid; the
     sRGB slope through powf evaluated at x +- ex, both branches admitted within ex of the knee), bf16: + half an ulp of the stored
     value.  Features 3..15 and the rows M .. Mpad - 1: exactly zero.
  b  directional chain: backward_ref.check_chain_layer / chain_tol per slot (16 from the head through spec_rgb_head, 15..9), judged with
     the mask RECORDS the kernel reads; d_allin = D13 W_dir2.0[:, :167] + D9 W_dir1.0: two K = 256 accumulations, the first stored
     (bf16: rounded to bf16), read back, added in fp32 and stored again:
        bf16: chain_tol(s1, a1) + 1.01 K u a2 + (2^-8 + 2 u) (|s1 + s2| + both)     fp32: (K + 2) u (a1 + a2) + u (|s1 + s2| + ...)
     The transposed layers are zero-padded from 167 to 192 rows, RowsOut writes all six 32-column blocks of every row m < M: columns
     167..191 are exactly zero (bf16: the conversion of 0 + 0).
  c  heads delta: the IDE backward over the 19 (m, l) terms, the reflection, the normalisation with its 1e-7, softplus', the sigmoid
     slopes and the sRGB slope, re-evaluated in fp64 operation by operation in the kernel's own order next to a running error bound
     (cancelling sums are charged to the sum of the absolute values of their terms); the forward quantities the kernel re-forms come
     from ref_forward_ref.dir_state.  K groups 0..7 are d_allin[:, :128] bit for bit; features 11..15 and the padding rows exactly zero.
  d  spatial chain: slot 7 from the 139 features [bottle-neck delta | 11 head rows] through H = [bottle_neck ; heads], 6..0: as b.
  e  the 20 + 20 parameter gradients: backward_ref.outer / wgrad_tol of the dumped delta rows and the dumped activation rows; the
     column windows of spa_block2.0 (63 | 256), dir_block1.0 (128 | 39) and dir_block2.0 (128 | 39 | 256) are separate products with
     separate bounds; the 9 + 2 head rows in the reference's row order.
  f  density gradient: d_enc from the mask records alone -- no delta of this chain is stored, so the bound is PROPAGATED: the
     rounding of every slot is carried to d_enc through the chain's own per-sample linear map (denc_ref); in bf16 that worst case is
     as large as the signal, so d_enc is ALSO judged against the slots the parameter chain stores under a unit density gradient
     (denc_rows_ref: one fp32 row accumulation); the rows are fp32 accumulators (no conversion).  The
     (M, 3) output is then judged against the d_enc the kernel left in the workspace: acc = d_c + sum_f 2^f (cos d_sin - sin d_cos) with
     sincos_quadrant at 4 u (ref_forward_ref.PE_C32), the contraction x (2 - 1/r) / r and its Jacobian k g + (1 / r^2 - k) (u.g) u by
     the running analysis; within the norm's error of r = 1 the difference of the two branches is admitted (both are the identity there).

No constant is measured on the code under test; none rests on a CPU-measured libm figure (division, expf, log1pf, sqrtf, powf: the
device library's documented ulp figures ref_forward_ref already uses)."""
import torch

import backward_ref as R
import forward_ref as F
import ref_forward_ref as RR
from ref_forward_ref import HALF, TINY, TL, TM, U, _add, _count, _div, _fma, _mul, _norm3, _report, _sigmoid, _stored, _zero

N_SLOTS = RR.N_SLOTS
DIR_SLOTS, SPA_SLOTS = (16, 15, 14, 13, 12, 11, 10, 9), (7, 6, 5, 4, 3, 2, 1, 0)
HEAD_ROWS_NCT, HEAD_ROWS_RT = (0, 1, 2, 4, 5, 6, 8, 9, 10), (3, 7)      # kernel head rows -> norm_col_tint_head rows 0..8, rho_tau_head rows 0..1
S8D_WIDTH = 160                                                          # the ten K groups of delta slot 8 that are written
EXACT = ("spec-zero", "heads-zero", "bn-order", "dallin-pad", "off-nonzero", "denc-pad")
C_Q = RR.f32c(-0.5833333333333333)
C_SLOPE = float((torch.tensor(211.0, dtype=torch.float32) / torch.tensor(200.0, dtype=torch.float32) *
                 torch.tensor(0.4166666666666667, dtype=torch.float32)).double())


def align256(n):
    return (n + 255) // 256 * 256


def dallin_offset(prec, M):
    """byte offset of d_allin in bwd_ref_backward's workspace"""
    return align256(N_SLOTS * F.geometry(prec, M)[1])


def partials_offset(prec, M):
    return dallin_offset(prec, M) + align256(M * 192 * 4)


def dallin_rows(ws, prec, M):
    """the workspace (uint8, base 256-aligned) -> d_allin (M, 192) in the element type the kernels use for it"""
    off = dallin_offset(prec, M)
    if prec == "bf16":
        return ws[off: off + M * 192 * 2].view(torch.bfloat16).view(M, 192)
    return ws[off: off + M * 192 * 4].view(torch.float32).view(M, 192)


def m_pad(prec, M):
    return F.geometry(prec, M)[0] * 32


# ------------------------------------------------------------------------------------------------ element-wise stages
def _c(x, like):
    return torch.full_like(like, x)


def srgb_slope_ref(x, ex):
    """(value, error) of srgb_slope(x): 12.92 below the knee, (211 / 200 * 5 / 12) powf(max(2^-23, x), -7 / 12) above"""
    o = _zero(x)
    m = x.clamp_min(RR.C_EPS)
    p = m ** C_Q
    lo, hi = (m + ex) ** C_Q, (m - ex).clamp_min(RR.C_EPS) ** C_Q          # (decreasing in x)
    ep = torch.maximum(hi - p, p - lo) + RR.POW_C * U * hi
    s1 = _mul(_c(C_SLOPE, x), o, p, ep)
    below = x <= RR.C_KNEE
    want, tol = torch.where(below, _c(RR.C_1292, x), s1[0]), torch.where(below, o, s1[1])
    near = (x - RR.C_KNEE).abs() <= ex
    return want, torch.where(near, s1[1] + (RR.C_1292 - s1[0]).abs(), tol)


def _linear_colour(a, c):
    o = _zero(a[:, 0])
    dd = _add(a[:, 4 + c], o, _c(-RR.C_LOG3, o), o)
    return _add(*_mul(*_sigmoid(a[:, 11 + c], o), *_sigmoid(a[:, 8 + c], o)), *_sigmoid(*dd))


def _g_slope(g, a, c, flags):
    """(value, error) of g_c * f'(linear colour of channel c)"""
    o = _zero(g)
    if not flags & RR.REF_SRGB:
        return g, o                                                           # (g * 1.0f is exact)
    return _mul(g, o, *srgb_slope_ref(*_linear_colour(a, c)))


def _dsig(s):
    """(value, error) of s (1 - s) from the pair of s"""
    return _mul(*s, *_add(torch.ones_like(s[0]), _zero(s[0]), -s[0], s[1]))


def spec_head_ref(g_out, aux, flags):
    """-> (value (M, 3), error (M, 3)) of the spec head's delta before it is stored"""
    g, a = g_out.double(), aux.double()
    o = _zero(a[:, 0])
    cols = []
    for c in range(3):
        sp, st = _sigmoid(a[:, 11 + c], o), _sigmoid(a[:, 8 + c], o)
        cols.append(_mul(*_mul(*_g_slope(g[:, c], a, c, flags), *st), *_dsig(sp)))
    return torch.stack([v for v, _ in cols], 1), torch.stack([e for _, e in cols], 1)


def heads_delta_ref(g_out, aux, dirs, d_allin, table, flags):
    """-> (value (M, 11), error (M, 11)) of the head rows' delta in the kernel's row order, from the (M, 192) rows d_allin as stored"""
    g, a, da, d = g_out.double(), aux.double(), d_allin.double(), dirs.double()
    st = RR.dir_state(aux, dirs)
    o = _zero(a[:, 0])
    comp, nn, dot, zp, re, im, att = st["comp"], st["nn"], st["dot"], st["zp"], st["re"], st["im"], st["att"]
    mat = table.double()
    d_re, d_im, d_rz, d_kinv = [(o, o)] * 9, [(o, o)] * 9, (o, o), (o, o)
    for t in range(19):
        mm, l = TM[t], TL[t]
        poly, dpoly = (o, o), (o, o)
        for k in range(l - mm + 1):
            poly = _fma(mat[k, t].expand_as(o), o, *zp[k], *poly)
            if k >= 1:
                dpoly = _fma(_c(RR.f32c(float(k) * float(mat[k, t])), o), o, *zp[k - 1], *dpoly)     # ((float)k * mat: one rounded product)
        gr, gi = (da[:, 128 + t], o), (da[:, 147 + t], o)
        A = _add(*_mul(*gr, *re[mm]), *_mul(*gi, *im[mm]))
        d_rz = _add(*d_rz, *_mul(*_mul(*A, *att[l]), *dpoly))
        tk = _mul(*_mul(*_mul(*A, *poly), _c(RR.SIGMA[l], o), o), *att[l])
        d_kinv = _add(*d_kinv, -tk[0], tk[1])
        d_re[mm] = _add(*d_re[mm], *_mul(*_mul(*gr, *poly), *att[l]))
        d_im[mm] = _add(*d_im[mm], *_mul(*_mul(*gi, *poly), *att[l]))
    d_rx, d_ry = (o, o), (o, o)
    for k in range(1, 9):
        kk = _c(float(k), o)
        p, q = _mul(*d_re[k], *re[k - 1]), _mul(*d_im[k], *im[k - 1])
        d_rx = _add(*d_rx, *_mul(kk, o, *_add(*p, *q)))
        p, q = _mul(*d_im[k], *re[k - 1]), _mul(*d_re[k], *im[k - 1])
        d_ry = _add(*d_ry, *_mul(kk, o, *_add(p[0], p[1], -q[0], q[1])))
    d_r = (d_rx, d_ry, d_rz)
    g_nd = (da[:, 166], o)
    rdotn = _add(*_add(*_mul(*d_rx, *comp[0]), *_mul(*d_ry, *comp[1])), *_mul(*d_rz, *comp[2]))
    dn = []
    for c in range(3):
        t1 = _add(g[:, 4 + c], o, *_mul(*g_nd, d[:, c], o))
        inner = _add(*_mul(*rdotn, d[:, c], o), *_mul(*dot, *d_r[c]))
        dn.append(_add(*t1, -2.0 * inner[0], 2.0 * inner[1]))
    n0 = [a[:, c] for c in range(3)]
    n0dn = _add(*_add(*_mul(n0[0], o, *dn[0]), *_mul(n0[1], o, *dn[1])), *_mul(n0[2], o, *dn[2]))
    ln = _norm3(*n0)
    ln = (ln[0].clamp_min(1e-30), ln[1])
    cden = _div(*n0dn, *_mul(*_mul(*ln, *nn), *nn))
    dh = []
    for c in range(3):
        q, p = _div(*dn[c], *nn), _mul(n0[c], o, *cden)
        v = _add(*q, -p[0], p[1])
        dh.append((-v[0], v[1]))
    dh.append(_mul(*d_kinv, *_sigmoid(*_add(a[:, 3], o, _c(-1.0, o), o))))
    dif, tint = [], []
    for c in range(3):
        sd = _sigmoid(*(_add(a[:, 4 + c], o, _c(-RR.C_LOG3, o), o) if flags & RR.REF_SRGB else (a[:, 4 + c], o)))
        stt, sp = _sigmoid(a[:, 8 + c], o), _sigmoid(a[:, 11 + c], o)
        gl = _g_slope(g[:, c], a, c, flags)
        dif.append(_mul(*gl, *_dsig(sd)))
        tint.append(_mul(*_mul(*gl, *sp), *_dsig(stt)))
    dh = dh + dif + [(g[:, 3], o)] + tint
    return torch.stack([v for v, _ in dh], 1), torch.stack([e for _, e in dh], 1)


def _nonzero(*parts):
    return {"worst": float(sum(int((p != 0).sum()) for p in parts)), "where": None, "neg_nonzero": 0}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_elementwise(prec, run, table, flags):
    """stages a and c.  run: s8d (Mpad, 160) rows of delta slot 8 up to the end of the last tile, d_allin (M, 192), aux, dirs, g_out"""
    s8d, da, aux = run["s8d"], run["d_allin"], run["aux"]
    M = aux.shape[0]
    rep = {}
    want, err = spec_head_ref(run["g_out"], aux, flags)
    rep["spec-head"] = _report(s8d[:M, 144:147], want, _stored(want, err, prec))
    rep["spec-zero"] = _nonzero(s8d[:M, 147:160], s8d[M:, 144:160])
    want, err = heads_delta_ref(run["g_out"], aux, run["dirs"], da.float(), table, flags)
    rep["heads-delta"] = _report(s8d[:M, 128:139], want, _stored(want, err, prec))
    rep["heads-delta"]["where"] = (rep["heads-delta"]["where"][0], 128 + rep["heads-delta"]["where"][1])
    rep["heads-zero"] = _nonzero(s8d[:M, 139:144], s8d[M:, :144])
    assert da.dtype == s8d.dtype
    rep["bn-order"] = _count(_bits(s8d[:M, :128]) != _bits(da[:, :128]))
    return rep


# ------------------------------------------------------------------------------------------------ chains
def operands(ws, prec):
    """the 19 master matrices pack_ref / pack_ref_bwd take (ref_forward_ref.kernel_tensors) as the chains multiply them -> fp64"""
    return [R.operand(w, prec) for w in ws[:19]]


def dir_stage(L, head3, deltas, w):
    """-> (d_in (M, K), W (K, N)) with delta_L = (d_in . W) * mask_L for the directional chain"""
    if L == 16:
        return head3, w[18]
    if L == 12:
        return deltas[13], w[14][:, 167:]
    return deltas[L + 1], w[L + 2]                               # slot 9 + i = output of tensor 10 + i; delta_L comes through tensor L + 2


def spa_stage(L, s8d, deltas, w):
    if L == 7:
        return s8d[:, :139], torch.cat((w[8], w[9]), 0)
    if L == 3:
        return deltas[4], w[4][:, 63:]
    return deltas[L + 1], w[L + 1]


def dallin_tol(s1, a1, s2, a2, K, prec):
    if prec == "bf16":
        t = R.chain_tol(s1, a1, K, "bf16") + 1.01 * K * U * a2 + K * TINY
        return t + (HALF + 2.0 * U) * ((s1 + s2).abs() + t)
    t = (K + 2) * U * (a1 + a2) + 2 * K * TINY
    return t + U * ((s1 + s2).abs() + t)


def _chain_rep(rep):
    return {"worst": rep["worst"], "where": rep["where"], "neg_nonzero": rep["off_nonzero"], "on_zero": rep["on_zero"]}


def check_chains(prec, w, run):
    """stages b and d.  run: deltas {slot: rows} for the 16 hidden slots, s8d, masks {slot: bool rows}, d_allin; w = operands(...)"""
    deltas, s8d, masks, da = run["deltas"], run["s8d"], run["masks"], run["d_allin"]
    M = da.shape[0]
    s8d = s8d[:M]
    rep, off = {}, 0
    for L in DIR_SLOTS:
        d_in, wm = dir_stage(L, s8d[:, 144:147], deltas, w)
        r = R.check_chain_layer(deltas[L], d_in, wm, masks[L][:M], prec)
        rep["D%d" % L] = _chain_rep(r)
        off += r["off_nonzero"]
    s1, a1 = R.contract(deltas[13], w[14][:, :167])
    s2, a2 = R.contract(deltas[9], w[10])
    rep["dallin"] = _report(da[:, :167], s1 + s2, dallin_tol(s1, a1, s2, a2, 256, prec))
    rep["dallin-pad"] = _count(da[:, 167:].float() != 0)
    for L in SPA_SLOTS:
        d_in, wm = spa_stage(L, s8d, deltas, w)
        r = R.check_chain_layer(deltas[L], d_in, wm, masks[L][:M], prec)
        rep["S%d" % L] = _chain_rep(r)
        off += r["off_nonzero"]
    rep["off-nonzero"] = {"worst": float(off), "where": None, "neg_nonzero": 0}
    return rep


# ------------------------------------------------------------------------------------------------ parameter gradients
def grad_refs(prec, run, n_wg, rows=None, prod=None):
    """-> {name: (fp64 value, tol)} for w0..w19 / b0..b19 in ops.ref_backward's order.  run: deltas, s8d, acts {slot: rows}, s8 = the
    ACTIVATION slot 8 rows (M, 240).  rows = index tensor of the samples that may be nonzero (comb regime)."""
    M = run["s8"].shape[0]
    pick = (lambda t: t[:M]) if rows is None else (lambda t: t[rows])
    deltas, acts = {k: pick(v) for k, v in run["deltas"].items()}, {k: pick(v) for k, v in run["acts"].items()}
    s8d = pick(run["s8d"])
    bn, ide39, ex = (pick(t) for t in RR.split_slot8(run["s8"]))
    n_nz = int((s8d != 0).any(dim=1).sum())
    out = {}

    def ref_prod(d, x):
        s, a = R.outer(d, x)
        return s, R.wgrad_tol(a, n_nz, n_wg, prec)
    prod = prod or ref_prod                                      # (the host emulation passes its own fp32 product and gets the same table)

    def put(i, d, xs):
        parts = [prod(d, x) for x in xs]
        out["w%d" % i] = (torch.cat([p[0] for p in parts], 1), None if parts[0][1] is None else torch.cat([p[1] for p in parts], 1))
        out["b%d" % i] = prod(d, None)
    put(0, deltas[0], [ex])
    for l in (1, 2, 3, 5, 6, 7):
        put(l, deltas[l], [acts[l - 1]])
    put(4, deltas[4], [ex, acts[3]])
    heads = s8d[:, 128:139]
    put(8, s8d[:, :128], [acts[7]])
    put(9, heads[:, list(HEAD_ROWS_NCT)], [acts[7]])
    put(10, heads[:, list(HEAD_ROWS_RT)], [acts[7]])
    put(11, deltas[9], [bn, ide39])
    for l in (1, 2, 3, 5, 6, 7):
        put(11 + l, deltas[9 + l], [acts[8 + l]])
    put(15, deltas[13], [bn, ide39, acts[12]])
    put(19, s8d[:, 144:147], [acts[16]])
    return out


# ------------------------------------------------------------------------------------------------ density gradient
def rows_tol(a, K, prec):
    """an fp32 row output of K accumulated products (bf16 operands: exact products)"""
    return (1.01 * K if prec == "bf16" else K + 2) * U * a + K * TINY


def _denc_tables(net, w):
    if net == "ref":
        return 7, w[9][7:8], {6: w[7], 5: w[6], 4: w[5], 3: w[4][:, 63:], 2: w[3], 1: w[2], 0: w[1]}, {4: w[4][:, :63], 0: w[0]}
    return 3, w[4], {2: w[3], 1: w[2], 0: w[1]}, {0: w[0]}


def _denc_chunk(top, head, layers, outs, spec, masks, prec):
    m = {L: masks[L].double() for L in range(top + 1)}
    d = {top: head.double() * m[top]}                             # (1.0 x w: exact in either precision)
    e = torch.zeros(d[top].shape[0], dtype=torch.float64, device=d[top].device)
    rho, e_at = {}, {top: e}
    for L in range(top - 1, -1, -1):
        wd = layers[L].double()
        s, a = d[L + 1] @ wd, d[L + 1].abs() @ wd.abs()
        dev = e[:, None] * wd.norm(dim=0)[None, :]
        rho[L] = R.chain_tol(s.abs() + dev, a + dev, 256, prec) * m[L]
        d[L] = s * m[L]
        e = spec[L] * e + rho[L].norm(dim=1)
        e_at[L] = e
    want, tol = None, None
    for L in sorted(outs, reverse=True):
        ad = outs[L].double()
        s, a = d[L] @ ad, d[L].abs() @ ad.abs()
        t = rows_tol(a + e_at[L][:, None] * ad.norm(dim=0)[None, :], 256, prec)
        if want is None:
            want, tol = s, t
        else:
            want = want + s
            tol = tol + t + U * (want.abs() + tol + t)
    V = None
    n = m[0].shape[0]
    for L in range(top):
        if L:                                                     # one GEMM over all samples: W (256, 256) x (256, n 63)
            X = (m[L - 1][:, :, None] * V).permute(1, 0, 2).reshape(256, n * 63)
            V = (layers[L - 1].double() @ X).reshape(256, n, 63).permute(1, 0, 2)
        else:
            V = None
        if L in outs:
            A = outs[L].double()[None].expand(m[0].shape[0], -1, -1)
            V = A if V is None else V + A
        tol = tol + (rho[L][:, :, None] * V.abs()).sum(1)
    return want, tol


def denc_ref(net, prec, w, masks, chunk=2048):
    """d density / d (encoded position) from the mask records alone -> (value (M, 63), bound (M, 63)) in the reference's column order.
    net 'ref': w = operands(...) of the 19 tensors, masks {0..7}; net 'prop': w = the five operand matrices, masks {0..3}.

    No delta of this chain is stored, so the bound is propagated -- through the chain's own linear map, not through |W| (which grows
    by the cancellation factor a / |s| ~ 13 per layer and ends 10^3 .. 10^4 times above the signal).  With the masks fixed the chain is
    linear, so (computed - exact) d_enc = sum_L J_L rho_L EXACTLY, J_L = the per-sample map from slot L to d_enc and rho_L the rounding
    committed at slot L: |rho_L| <= chain_tol(|s^|, a^) of the COMPUTED operands, zero where the mask bit is clear.  First order:
    sum_L |J_L| chain_tol(s_L, a_L), |J_L| (256 x 63 per sample) by the recurrence J_L = W diag(mask_{L-1}) J_{L-1} (+ the skip
    layer's own columns).  Second order (the computed operands differ from the exact ones): |s^ - s|_j, |a^ - a|_j <= e |W[:, j]|_2
    (Cauchy-Schwarz) with e >= |computed - exact delta|_2 from e_L = |W|_2 e_{L+1} + |rho_L|_2."""
    top, head, layers, outs = _denc_tables(net, w)
    spec = {L: float(torch.linalg.matrix_norm(layers[L].double(), 2)) for L in layers}
    M = masks[0].shape[0]
    want, tol = [], []
    for i in range(0, M, chunk):
        a, b = _denc_chunk(top, head, layers, outs, spec, {L: masks[L][i: i + chunk] for L in range(top + 1)}, prec)
        want.append(a); tol.append(b)
    return torch.cat(want), torch.cat(tol)


def denc_rows_ref(net, prec, w, deltas):
    """d_enc from STORED delta rows: the parameter chain of the same network run with a unit density gradient (Ref-NeRF: g_out = e_3,
    whose spec head, directional chain, d_allin and every head row but the density's are exact zeros; proposal: g_density = 1) forms
    slot by slot what the density-gradient chain forms -- same operands (the second copies of the layers in the stream), the same
    `dense` K order, one conversion per slot -- and stores it.  d_enc is then one (two) K = 256 fp32 row accumulation(s) of slots 0
    (and 4): rows_tol, the sharp companion of denc_ref, whose worst case over seven unstored bf16 layers is as large as the signal."""
    _, _, _, outs = _denc_tables(net, w)
    want, tol = None, None
    for L in sorted(outs, reverse=True):
        s, a = R.contract(deltas[L], outs[L])
        t = rows_tol(a, 256, prec)
        if want is None:
            want, tol = s, t
        else:
            want = want + s
            tol = tol + t + U * (want.abs() + tol + t)
    return want, tol


def _sincos(a, ea):
    e = RR.PE_C32 * U + ea
    return (torch.sin(a), e), (torch.cos(a), e)


def pe_grad_ref(d_enc, x, scale, contract):
    """(value (M, 3), bound (M, 3)) of pe_grad_kernel / pe_grad_contract_kernel from the d_enc rows (M, >= 63) as the chain left them"""
    d, x = d_enc.double(), x.double()[:, :3]
    o = _zero(x[:, 0])
    one = torch.ones_like(o)
    xs = [(x[:, c], o) for c in range(3)]
    if contract:
        r = _norm3(x[:, 0], x[:, 1], x[:, 2])
        outside, edge = r[0] > 1.0, (r[0] - 1.0).abs() <= r[1]
        rs = (r[0].clamp_min(TINY), r[1])
        inv = _div(one, o, *rs)
        k = _div(*_add(2.0 * one, o, -inv[0], inv[1]), *rs)
        cx = [_mul(*xs[c], *k) for c in range(3)]
    branches = []
    for pos in ([xs] + ([cx] if contract else [])):
        g = []
        for c in range(3):
            acc = (d[:, c], o)
            for f in range(10):
                fr = 2.0 ** f
                sn, cs = _sincos(pos[c][0] * fr, pos[c][1] * fr)
                p, q = _mul(*cs, d[:, 3 + 6 * f + c], o), _mul(*sn, d[:, 6 + 6 * f + c], o)
                t = _add(p[0], p[1], -q[0], q[1])
                acc = _add(*acc, fr * t[0], fr * t[1])
            g.append(acc)
        branches.append(g)
    g = branches[0]
    if contract:
        gc = branches[1]
        u = [_div(*xs[c], *rs) for c in range(3)]
        ug = _add(*_add(*_mul(*u[0], *gc[0]), *_mul(*u[1], *gc[1])), *_mul(*u[2], *gc[2]))
        ir = _div(one, o, *_mul(*rs, *rs))
        t = _mul(*ug, *_add(*ir, -k[0], k[1]))
        out = []
        for c in range(3):
            v = _add(*_mul(*k, *gc[c]), *_mul(*t, *u[c]))
            inside = g[c]
            val = torch.where(outside, v[0], inside[0])
            err = torch.where(outside, v[1], inside[1])
            err = torch.where(edge, torch.maximum(v[1], inside[1]) + (v[0] - inside[0]).abs(), err)
            out.append((val, err))
        g = out
    if scale is not None:
        g = [_mul(*g[c], scale.double(), o) for c in range(3)]
    return torch.stack([v for v, _ in g], 1), torch.stack([e for _, e in g], 1)


def check_density_grad(net, prec, w, masks, d_enc, x, scale, contract, out, deltas=None):
    """stage f.  d_enc (M, 64) fp32 = the rows in the workspace, out (M, 3) = the entry point's result; deltas = the stored slots of
    the parameter chain under a unit density gradient (denc_rows_ref) or None"""
    M = out.shape[0]
    rep = {"denc-pad": _count(d_enc[:, 63:] != 0)}
    if masks is not None:                                         # (per-sample 256 x 63 maps: the caller leaves it out at very large M)
        want, tol = denc_ref(net, prec, w, {L: v[:M] for L, v in masks.items()})
        rep["denc"] = _report(d_enc[:, :63], want, tol)
    if deltas is not None:
        want, tol = denc_rows_ref(net, prec, w, {L: v[:M] for L, v in deltas.items()})
        rep["denc-rows"] = _report(d_enc[:, :63], want, tol)
    want, tol = pe_grad_ref(d_enc, x, scale, contract)
    rep["pe-grad"] = _report(out, want, tol)
    return rep


# ------------------------------------------------------------------------------------------------ reports
def limit(stage):
    return 0.0 if stage in EXACT else 1.0


def ratios(rep):
    out = {}
    for k, v in rep.items():
        out[k] = v["worst"]
        if v.get("neg_nonzero") and k not in EXACT:
            out[k] = float("inf")                                  # a delta on a switched-off unit fails its layer outright
    return out


def failing(rep):
    return sorted(k for k, v in ratios(rep).items() if not v <= limit(k))


def assert_report(what, rep):
    bad = failing(rep)
    assert not bad, "%s: beyond the bound in %s" % (what, ", ".join("%s (%.3g at %s)" % (k, rep[k]["worst"], rep[k]["where"]) for k in bad))


# ------------------------------------------------------------------------------------------------ honest emulation (host test)
def _f(x):
    return torch.tensor(x, dtype=torch.float32)


def _sig32(v):
    return 1.0 / (1.0 + torch.exp(-v))


def _slope32(a, c, flags):
    if not flags & RR.REF_SRGB:
        return torch.ones_like(a[:, 0])
    x = _sig32(a[:, 11 + c]) * _sig32(a[:, 8 + c]) + _sig32(a[:, 4 + c] - _f(1.0986122886681098))
    hi = (_f(211.0) / _f(200.0)) * _f(0.4166666666666667) * torch.maximum(_f(RR.C_EPS), x) ** _f(-0.5833333333333333)
    return torch.where(x <= _f(0.0031308), _f(12.92).expand_as(x), hi)


def heads_delta_f32(g, a, d, da, table, flags, fault=None):
    """ref_heads_delta_kernel's per-sample arithmetic in fp32, operation by operation -> (M, 11)"""
    n0 = a[:, 0:3]
    ln = torch.sqrt((n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1]) + n0[:, 2] * n0[:, 2])
    nn = ln + _f(1e-7)
    n = -n0 / nn[:, None]
    dot = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    r = d - (2.0 * dot)[:, None] * n
    kinv = torch.nn.functional.softplus(a[:, 3] - 1.0)
    one, zero = torch.ones_like(ln), torch.zeros_like(ln)
    zp, re, im = [one], [one], [zero]
    for k in range(1, 9):
        zp.append(zp[k - 1] * r[:, 2])
        re.append(re[k - 1] * r[:, 0] - im[k - 1] * r[:, 1])
        im.append(re[k - 1] * r[:, 1] + im[k - 1] * r[:, 0])
    att = {l: torch.exp(-s * kinv) for l, s in RR.SIGMA.items()}
    d_re, d_im, d_rz, d_kinv = [zero] * 9, [zero] * 9, zero, zero
    for t in range(19):
        mm, l = TM[t], TL[t]
        poly, dpoly = zero, zero
        for k in range(l - mm + 1):
            poly = RR._fma32(table[k, t].expand_as(one), zp[k], poly)
            if k >= 1:
                dpoly = RR._fma32((float(k) * table[k, t]).expand_as(one), zp[k - 1], dpoly)
        gr, gi = da[:, 128 + t], da[:, 147 + t]
        A = gr * re[mm] + gi * im[mm]
        term = A * att[l] * dpoly
        d_rz = d_rz + (-term if (fault == "ide_sign" and t == 7) else term)
        d_kinv = d_kinv - A * poly * RR.SIGMA[l] * att[l]
        d_re[mm] = d_re[mm] + gr * poly * att[l]
        d_im[mm] = d_im[mm] + gi * poly * att[l]
    d_rx, d_ry = zero, zero
    for k in range(1, 9):
        d_rx = d_rx + float(k) * (d_re[k] * re[k - 1] + d_im[k] * im[k - 1])
        d_ry = d_ry + float(k) * (d_im[k] * re[k - 1] - d_re[k] * im[k - 1])
    d_r = (d_rx, d_ry, d_rz)
    g_nd = da[:, 166]
    rdotn = (d_rx * n[:, 0] + d_ry * n[:, 1]) + d_rz * n[:, 2]
    two = 1.0 if fault == "refl2" else 2.0
    dn = [g[:, 4 + c] + g_nd * d[:, c] - two * (rdotn * d[:, c] + dot * d_r[c]) for c in range(3)]
    n0dn = (n0[:, 0] * dn[0] + n0[:, 1] * dn[1]) + n0[:, 2] * dn[2]
    cden = n0dn / (ln.clamp_min(1e-30) * nn * nn)
    dh = [-(dn[c] / nn - n0[:, c] * cden) for c in range(3)]
    dh.append(d_kinv * _sig32(a[:, 3] - 1.0))
    dif, tint = [], []
    for c in range(3):
        sd = _sig32(a[:, 4 + c] - _f(1.0986122886681098)) if flags & RR.REF_SRGB else _sig32(a[:, 4 + c])
        stt, sp = _sig32(a[:, 8 + c]), _sig32(a[:, 11 + c])
        gl = g[:, c] * _slope32(a, c, flags)
        dif.append(gl * (sd * (1.0 - sd)))
        tint.append(gl * sp * (stt * (1.0 - stt)))
    return torch.stack(dh + dif + [g[:, 3]] + tint, 1)


def emulate(prec, ws, fwd, dirs, g_out, table, flags=0, fault=None):
    """bwd_ref_backward's arithmetic on the CPU, honestly, on a forward run of ref_forward_ref.emulate (fwd: acts, s8, aux, masks): fp32
    chains (torch's order), one round-to-nearest conversion per stored element.  ws = the 19 fp32 masters.  -> run dict of the checks +
    'grads' {name: tensor}.  fault: a planted fault (tests/test_ref_backward_ref_host.py)."""
    cast = lambda v: R.element(v, prec)
    w = [R.operand(t, prec).float() for t in ws[:19]]
    acts, aux, masks = fwd["acts"], fwd["aux"].float(), fwd["masks"]
    M = aux.shape[0]
    Mp = m_pad(prec, M)
    g, d = g_out.float(), dirs.float()
    s8d = torch.zeros(Mp, S8D_WIDTH)
    for c in range(3):
        sp = _sig32(aux[:, 11 + c])
        s8d[:M, 144 + c] = (g[:, c] * _slope32(aux, c, flags)) * _sig32(aux[:, 8 + c]) * (sp * (1.0 - sp))
    s8d = cast(s8d)
    deltas = {}
    for L in DIR_SLOTS:
        d_in, wm = dir_stage(L, s8d[:M, 144:147], deltas, w)
        deltas[L] = cast((d_in.float() @ wm) * masks[L])
    v1, v2 = deltas[13].float() @ w[14][:, :167], deltas[9].float() @ w[10]
    da = torch.zeros(M, 192)
    da[:, :167] = cast(cast(v1).float() + v2).float() if prec == "bf16" else v1 + v2
    if fault == "skipblock":                                                     # the second side output lands one 32-column block further
        da[:, :167] = cast(v1).float()
        da[:, 32:] = cast(da[:, 32:] + torch.nn.functional.pad(v2, (0, 25))[:, :160]).float()
    da = cast(da)
    read = da.float()
    if fault == "bf16_as_fp32" and prec == "bf16":                                # the bf16 rows read through a float pointer with ld 192
        raw = torch.zeros(M * 192 * 2, dtype=torch.bfloat16)
        raw[: M * 192] = da.reshape(-1)
        read = raw.view(torch.float32).view(M, 192)
    s8d = s8d.float()
    s8d[:M, 128:139] = heads_delta_f32(g, aux, d, read, table.float(), flags, fault)
    s8d[:M, :128] = da[:, :128].float()
    s8d = cast(s8d)
    for L in SPA_SLOTS:
        d_in, wm = spa_stage(L, s8d[:M], deltas, w)
        deltas[L] = cast((d_in.float() @ wm) * masks[L])
    run = {"deltas": deltas, "s8d": s8d, "masks": masks, "d_allin": da, "aux": aux, "dirs": d, "g_out": g, "acts": acts, "s8": fwd["s8"]}
    def prod32(dd, x):
        if x is None:
            return dd.float().sum(0), None
        return dd.float().t() @ x.float(), None
    run["grads"] = {k: v[0] for k, v in grad_refs(prec, run, 1, prod=prod32).items()}
    return run


def emulate_density(net, prec, ws, masks, x, scale, contract, fault=None):
    """bwd_density_grad on the CPU: the chain in fp32 with one conversion per layer, fp32 rows, the encoding's derivative operation by
    operation in fp32 -> (d_enc (M, 64), out (M, 3)).  ws = the fp32 masters (19 of Ref-NeRF / 5 of the proposal network)"""
    cast = lambda v: R.element(v, prec).float()
    w = [R.operand(t, prec).float() for t in ws]
    if net == "ref":
        top, head = 7, w[9][7:8]
        layers = {6: w[7], 5: w[6], 4: w[5], 3: w[4][:, 63:], 2: w[3], 1: w[2], 0: w[1]}
        outs = [(4, w[4][:, :63]), (0, w[0])]
    else:
        top, head, layers, outs = 3, w[4], {2: w[3], 1: w[2], 0: w[1]}, [(0, w[0])]
    d = {top: head * masks[top]}
    for L in range(top - 1, -1, -1):
        d[L] = cast(d[L + 1] @ layers[L]) * masks[L]
    M = x.shape[0]
    d_enc = torch.zeros(M, 64)
    for L, wm in outs:
        d_enc[:, :63] = d_enc[:, :63] + d[L] @ wm
    x = x.float()[:, :3]
    k = None
    pos = x
    if contract:
        r = torch.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        outside = r > 1.0
        k = torch.where(outside, (2.0 - 1.0 / r) / r, torch.ones_like(r))
        pos = x * k[:, None]
    g = []
    for c in range(3):
        acc = d_enc[:, c]
        for f in range(10):
            fr = float(1 << f)
            a = pos[:, c] * fr
            acc = acc + fr * (torch.cos(a) * d_enc[:, 3 + 6 * f + c] - torch.sin(a) * d_enc[:, 6 + 6 * f + c])
        g.append(acc)
    g = torch.stack(g, 1)
    if contract:
        u = x / r[:, None]
        ug = (u[:, 0] * g[:, 0] + u[:, 1] * g[:, 1]) + u[:, 2] * g[:, 2]
        t = ug * (1.0 / (r * r) - k)
        if fault == "uut":
            t = torch.zeros_like(t)
        g = torch.where(outside[:, None], k[:, None] * g + t[:, None] * u, g)
    if scale is not None:
        g = g * scale.float()[:, None]
    return d_enc, g
