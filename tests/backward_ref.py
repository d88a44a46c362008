"""fp64 references and worst-case element-wise bounds for the MLP training backward (nerf_amd/csrc/bwd_kernels.hip), one stage at a
time.  Plain helper module (no fixtures): tests/test_gpu_backward_layers.py feeds it the rows the kernels dumped, and
tests/test_backward_ref_host.py feeds it a torch fp64 forward and checks it against torch.autograd before it is trusted as a yardstick.

Every stage is compared AGAINST ITS OWN INPUTS: the delta of chain layer L from the dumped delta of layer L+1 and the dumped activation of
layer L, a weight gradient from the dumped delta and activation rows.  Masks and operands are then identical on both sides, and what is
left is the accumulation order and at most one rounding of the result.

Bounds (u = 2^-24, the fp32 unit roundoff; s = sum_k d_k w_k, A = sum_k |d_k w_k| formed in fp64 from the operands the kernel multiplies):

  chain layer, bf16:   |got - s| <= 2^-8 |s| + 1.01 K u A + K 2^-126
      the product of two bf16 numbers (8 significant bits each) is exact in fp32; adding K terms in ANY order, each addition rounded to
      fp32, is within ((1 + u)^(K - 1) - 1) A <= 1.01 (K - 1) u A of s for K <= 2^16; one round-to-nearest-even to bf16 (8 significant
      bits: half an ulp <= 2^-8 of the value) on top, applied to a value that itself is within the second term of s (the 1.01 K instead
      of 1.01 (K - 1) pays for the cross term); K 2^-126 covers products / partial sums flushed as subnormals.  A truncating conversion
      (error up to 2^-7 |s|) does not fit.
  chain layer, fp32:   |got - s| <= (K + 2) u A + K 2^-126
      K rounded products (or fused multiply-adds) and K - 1 rounded additions; no final conversion.
  weight / bias gradient (a contraction over samples):  tol = 1.01 (n_nz + n_wg + 8) u A + n_nz 2^-126   (+ 2 n_nz u A in fp32 mode)
      only the n_nz samples with a nonzero head delta contribute a nonzero term (adding an exact zero does not round), n_wg workgroup
      partials are added by the finalize kernel, 8 covers its fixed 4 x 4 combination tree; fp32 mode also rounds each product and runs
      the operand transposition through the matrix cores.  In the comb regime (n_nz <= 512) this is ~1e-4 A: far below one sample's share.
  un-folded tensors (mip_fold_grads_kernel, fp32 fused multiply-add chains over G = dc^T g6 and s = sum dc):
      bottle_neck.0      = W9a^T G        : |W9a|^T tol_G + 130 u |W9a|^T |G|
      bottle_neck.0 bias = W9a^T s        : |W9a|^T tol_s + 130 u |W9a|^T |s|
      rgb_layer.0[:, :256] = G Wb^T + s bb^T : tol_G |Wb|^T + tol_s |bb|^T + 258 u (|G| |Wb|^T + |s| |bb|^T)

None of these is fitted to what the kernels produce."""
import torch

U24 = 2.0 ** -24
TINY = 2.0 ** -126
BF16_HALF_ULP = 2.0 ** -8

TILE = {"bf16": 256, "fp32": 128}            # samples per backward tile (PBF16W: 4 waves x 2 x 32; PF32: 4 waves x 32)


# ------------------------------------------------------------------------------------------------ layout (mlp_layout.h)
def pe_slot_column(q, h, L):
    """column of the reference's [x | PE_L(x)] matrix that PE slot (q, h) holds, or -1 for zero padding"""
    if q < 3 * L:
        return 3 + 6 * (q // 3) + 3 * h + (q % 3)
    if q == 3 * L:
        return 2 if h else 0
    if q == 3 * L + 1:
        return -1 if h else 1
    return -1


def dmap_feature(kg, h, e):
    return 16 * kg + 8 * (e >> 2) + 4 * h + (e & 3)


def feature_slot(f):
    """inverse of dmap_feature: row feature f -> (K group, lane half, element)"""
    kg, r = divmod(f, 16)
    return kg, (r % 8) // 4, 4 * (r // 8) + (r % 4)


def enc_columns(n_kg, L):
    """reference column (or -1) of every feature of an encoding slot read as rows (16 n_kg features in D-map order)"""
    cols = []
    for f in range(16 * n_kg):
        kg, h, e = feature_slot(f)
        cols.append(pe_slot_column(8 * kg + e, h, L))
    return cols


def slot_to_reference(rows, L):
    """encoding slot rows (M, 16 n_kg) in slot order -> ((M, 3 + 6 L) in the reference's column order, the padding features)"""
    cols = enc_columns(rows.shape[1] // 16, L)
    used = [f for f, c in enumerate(cols) if c >= 0]
    assert sorted(cols[f] for f in used) == list(range(3 + 6 * L)), "the slot map is not a bijection onto the reference's columns"
    out = rows.new_zeros((rows.shape[0], 3 + 6 * L))
    out[:, [cols[f] for f in used]] = rows[:, used]
    pad = rows[:, [f for f, c in enumerate(cols) if c < 0]]
    return out, pad


def reference_to_slot(enc, L, n_kg):
    """the inverse (host test): reference-order columns -> slot-order rows with zero padding"""
    cols = enc_columns(n_kg, L)
    out = enc.new_zeros((enc.shape[0], 16 * n_kg))
    for f, c in enumerate(cols):
        if c >= 0:
            out[:, f] = enc[:, c]
    return out


def dump_element_offset(layer_stride, slot, m, f):
    """byte offset of feature f of sample m in slot `slot` of a bf16 fragment dump (slot, subtile, K group, lane, element)"""
    kg, h, e = feature_slot(f)
    return slot * layer_stride + ((m // 32) * 16 + kg) * 1024 + ((m % 32) + 32 * h) * 16 + e * 2


def mask_bit(m, f):
    """(byte offset inside a slot's mask block, bit) of feature f of sample m: 1 KiB per subtile, 16 B per lane, dword kg >> 2"""
    kg, h, e = feature_slot(f)
    lane = (m % 32) + 32 * h
    bit = 4 * (kg & 3) + (e >> 1) + 16 * (e & 1)
    return (m // 32) * 1024 + lane * 16 + (kg >> 2) * 4 + bit // 8, bit % 8


def decode_f8_slot(dump, layer, layer_stride, n_sub, n_kg=16):
    """host-side reading of one fp8 slot -> (n_sub * 32, 16 * n_kg) float32 rows (mlp_layout.h: 8 data blocks + scale exponents per subtile;
    element e of K group kg in lane j + 32 h = feature 16 kg + 8 (e >> 2) + 4 h + (e & 3) of sample j)"""
    raw = dump[layer * layer_stride: layer * layer_stride + n_sub * 9216].view(n_sub, 9216)
    data = raw[:, :8192].reshape(n_sub, 8, 64, 2, 8)                       # [sub][fb][lane][kg & 1][e]
    vals = data.view(torch.float8_e4m3fn).float()
    ex = raw[:, 8192:].reshape(n_sub, 64, 16).float()                      # [sub][lane][kg]
    scale = torch.exp2(ex - 127.0).permute(0, 2, 1).reshape(n_sub, 8, 2, 64).permute(0, 1, 3, 2)      # -> [sub][fb][lane][kg & 1]
    vals = vals * scale[..., None]
    v = vals.permute(0, 1, 3, 2, 4).reshape(n_sub, 16, 2, 32, 2, 4)        # [sub][kg][h][j][e >> 2][e & 3]
    rows = v.permute(0, 3, 1, 4, 2, 5).reshape(n_sub * 32, 16 * 16)        # feature = 16 kg + 8 (e >> 2) + 4 h + (e & 3)
    return rows[:, : 16 * n_kg]


# ------------------------------------------------------------------------------------------------ operands
def operand(w, prec):
    """a master weight as the kernels multiply it: fp32, or rounded to nearest-even to bf16 (pack_layer_kernel); -> fp64"""
    w = w.detach().float()
    return (w.to(torch.bfloat16) if prec == "bf16" else w).double()


def element(v, prec):
    """an fp32 value stored as a dump element"""
    return v.to(torch.bfloat16) if prec == "bf16" else v


def mip_head_f32(g_rgbo, rgbo):
    """the head K group of the MipNeRF chain as mip_bwd_kernel forms it in fp32: [(g * (1 - o)) * o | g_sigma]"""
    g, o = g_rgbo.float().reshape(-1, 4), rgbo.float().reshape(-1, 4)
    return torch.cat(((g[:, :3] * (1.0 - o[:, :3])) * o[:, :3], g[:, 3:4]), dim=1)


# ------------------------------------------------------------------------------------------------ layer tables
PROP_ORDER = (3, 2, 1, 0)
MIP_ORDER = (7, 6, 5, 4, 3, 2, 1, 0)
PROP_WIDTH = {0: 256, 1: 256, 2: 256, 3: 256}
MIP_WIDTH = {0: 256, 1: 256, 2: 256, 3: 256, 4: 256, 5: 256, 6: 256, 7: 128}
PROP_HEAD_SLOT, MIP_HEAD_SLOT = 4, 8


def prop_stage(L, head, deltas, w):
    """-> (d_in (M, K), W (K, N)) with delta_L = (d_in . W) * [act_L > 0]; w = the five operand matrices in state_dict order"""
    if L == 3:
        return head[:, :1], w[4]
    return deltas[L + 1], w[L + 1]


def mip_stage(L, head, deltas, w, w_fold):
    """w = the eleven operand matrices in MipNeRF._linear_layers() order, w_fold (128, 256) = rgb_layer.0[:, :256] . bottle_neck.0"""
    if L == 7:
        return head[:, :3], w[10]
    if L == 6:
        return torch.cat((deltas[7], head[:, 3:4]), dim=1), torch.cat((w_fold, w[8]), dim=0)
    if L == 3:
        return deltas[4], w[4][:, 63:]
    return deltas[L + 1], w[L + 1]


def stage(net, L, head, deltas, w, w_fold=None):
    return prop_stage(L, head, deltas, w) if net == "prop" else mip_stage(L, head, deltas, w, w_fold)


def contract(d, w, chunk=1 << 15):
    """fp64 s = d . w and A = |d| . |w| of (M, K) x (K, N), in row chunks"""
    s = torch.empty((d.shape[0], w.shape[1]), dtype=torch.float64, device=d.device)
    a = torch.empty_like(s)
    w64, wa = w.double(), w.double().abs()
    for i in range(0, d.shape[0], chunk):
        x = d[i: i + chunk].double()
        s[i: i + chunk] = x @ w64
        a[i: i + chunk] = x.abs() @ wa
    return s, a


def chain_tol(s, a, K, prec):
    if prec == "bf16":
        return BF16_HALF_ULP * s.abs() + 1.01 * K * U24 * a + K * TINY
    return (K + 2) * U24 * a + K * TINY


def check_chain_layer(got, d_in, w, act, prec, chunk=1 << 15):
    """One chain layer against its own inputs.  -> dict: worst = max(err / tol) over the elements whose activation is positive,
    where = (sample, feature) of it, off_nonzero = number of elements with act == 0 and a nonzero delta, on_zero = number of elements with
    act > 0, a zero delta and |s| beyond tol (what a mask bit that disagrees with the activation produces).  No element is exempt:
    a report passes only with worst <= 1 and off_nonzero == 0."""
    K, N = d_in.shape[1], got.shape[1]
    worst, where, off_nonzero, on_zero = 0.0, (0, 0), 0, 0
    w64, wa = w.double(), w.double().abs()
    for i in range(0, got.shape[0], chunk):
        x = d_in[i: i + chunk].double()
        s, a = x @ w64, x.abs() @ wa
        g = got[i: i + chunk].double()
        on = act[i: i + chunk] > 0
        off_nonzero += int(((~on) & (g != 0)).sum())
        tol = chain_tol(s, a, K, prec)
        ratio = torch.where(on, (g - s).abs() / tol, torch.zeros_like(s))
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        on_zero += int((on & (g == 0) & (ratio > 1)).sum())
        r = float(ratio.max())
        if r > worst:
            k = int(ratio.argmax())
            worst, where = r, (i + k // N, k % N)
    return {"worst": worst, "where": where, "off_nonzero": off_nonzero, "on_zero": on_zero}


def assert_chain_layer(name, rep):
    assert rep["off_nonzero"] == 0 and rep["worst"] <= 1.0, \
        "%s: max(err / tol) = %.3g at (sample, feature) %s; %d elements with act == 0 carry a delta, %d with act > 0 were zeroed" % (
            name, rep["worst"], rep["where"], rep["off_nonzero"], rep["on_zero"])


# ------------------------------------------------------------------------------------------------ weight gradients
def outer(d, x, chunk=1 << 15):
    """fp64 s = d^T x and A = |d|^T |x| of (M, No), (M, Ni); x = None: column sums (the bias gradient)"""
    no = d.shape[1]
    ni = 1 if x is None else x.shape[1]
    s = torch.zeros((no, ni), dtype=torch.float64, device=d.device)
    a = torch.zeros_like(s)
    for i in range(0, d.shape[0], chunk):
        dd = d[i: i + chunk].double()
        xx = torch.ones((dd.shape[0], 1), dtype=torch.float64, device=d.device) if x is None else x[i: i + chunk].double()
        s += dd.t() @ xx
        a += dd.abs().t() @ xx.abs()
    return (s[:, 0], a[:, 0]) if x is None else (s, a)


def wgrad_tol(a, n_nz, n_wg, prec):
    t = 1.01 * (n_nz + n_wg + 8) * U24 * a + TINY * n_nz
    return t + 2.0 * n_nz * U24 * a if prec == "fp32" else t


def prop_grad_refs(head, deltas, acts, enc, n_wg, prec, rows=None):
    """-> {name: (fp64 value, tol)} for the 5 + 5 tensors; acts[L] / deltas[L] = rows of slot L, enc = (M, 63) reference order.
    rows = index tensor of the samples that may be nonzero (comb regime: every other delta row was asserted to be exactly zero)."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    head, deltas, acts, enc = pick(head), {k: pick(v) for k, v in deltas.items()}, {k: pick(v) for k, v in acts.items()}, pick(enc)
    n_nz = int((head[:, :1] != 0).any(dim=1).sum())
    out = {}

    def put(name, d, x):
        s, a = outer(d, x)
        out[name] = (s, wgrad_tol(a, n_nz, n_wg, prec))
    put("w0", deltas[0], enc); put("b0", deltas[0], None)
    for L in (1, 2, 3):
        put("w%d" % L, deltas[L], acts[L - 1]); put("b%d" % L, deltas[L], None)
    put("w4", head[:, :1], acts[3]); put("b4", head[:, :1], None)
    return out


def mip_grad_refs(head, deltas, acts, enc, enc_d, w, b, n_wg, prec, rows=None):
    """-> {name: (fp64 value, tol)} for the 11 + 11 tensors (MipNeRF._linear_layers() order); acts[0..6] hidden, acts[7] = c (128),
    enc (M, 63) / enc_d (M, 27) in the reference's column order; w, b = the fp32 master parameters (the un-fold reads them as they are)."""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    head, enc, enc_d = pick(head), pick(enc), pick(enc_d)
    deltas, acts = {k: pick(v) for k, v in deltas.items()}, {k: pick(v) for k, v in acts.items()}
    n_nz = int((head[:, :4] != 0).any(dim=1).sum())
    out = {}

    def put(name, d, x):
        s, a = outer(d, x)
        out[name] = (s, wgrad_tol(a, n_nz, n_wg, prec))
        return out[name]
    put("w0", deltas[0], enc); put("b0", deltas[0], None)
    for L in (1, 2, 3, 5, 6):
        put("w%d" % L, deltas[L], acts[L - 1]); put("b%d" % L, deltas[L], None)
    (se, te), (sh, th) = put("w4e", deltas[4], enc), put("w4h", deltas[4], acts[3])       # two different products: encoding | hidden columns
    out["w4"] = (torch.cat((se, sh), dim=1), torch.cat((te, th), dim=1))
    del out["w4e"], out["w4h"]
    put("b4", deltas[4], None)
    put("w8", head[:, 3:4], acts[6]); put("b8", head[:, 3:4], None)
    put("w10", head[:, :3], acts[7]); put("b10", head[:, :3], None)
    G, tG = put("G", deltas[7], acts[6])
    sv, ts = put("b9", deltas[7], None)
    sd, td = put("w9d", deltas[7], enc_d)
    del out["G"], out["w9d"]
    W9a, Wb, bb = w[9].double()[:, :256], w[7].double(), b[7].double()
    out["w7"] = (W9a.t() @ G, W9a.abs().t() @ tG + 130 * U24 * (W9a.abs().t() @ G.abs()))
    out["b7"] = (W9a.t() @ sv, W9a.abs().t() @ ts + 130 * U24 * (W9a.abs().t() @ sv.abs()))
    s9 = G @ Wb.t() + sv[:, None] * bb[None, :]
    t9 = tG @ Wb.abs().t() + ts[:, None] * bb.abs()[None, :] + 258 * U24 * (G.abs() @ Wb.abs().t() + sv.abs()[:, None] * bb.abs()[None, :])
    out["w9"] = (torch.cat((s9, sd), dim=1), torch.cat((t9, td), dim=1))
    return out


def grad_ratios(refs, got):
    """{name: max(err / tol)} over every element of every tensor; got = {name: tensor}"""
    rep = {}
    for name, (s, tol) in refs.items():
        g = got[name].double().reshape(s.shape)
        bad = ~torch.isfinite(g)
        r = (g - s).abs() / tol
        rep[name] = float("inf") if bool(bad.any()) else (float(r.max()) if r.numel() else 0.0)
    return rep


def assert_grads(what, rep):
    bad = {k: v for k, v in rep.items() if not v <= 1.0}
    assert not bad, "%s: max(err / tol) beyond 1 in %s" % (what, ", ".join("%s (%.3g)" % kv for kv in sorted(bad.items())))


def named_grads(gw, gb):
    out = {"w%d" % i: t for i, t in enumerate(gw)}
    out.update({"b%d" % i: t for i, t in enumerate(gb)})
    return out


# ------------------------------------------------------------------------------------------------ comb probes
def comb_runs(M, tile, max_probes=512):
    """Lists of sample indices, at most `max_probes` each and at most one per 32-sample subtile inside a list, at varying lane positions,
    which together hit every subtile that holds a sample m < M, sample 0, sample M - 1 and the samples either side of every tile boundary."""
    n_sub = (M + 31) // 32
    passes = []
    for p in range(2):
        probes = []
        for s in range(n_sub):
            lane = (7 * s + 3 + 13 * p) % 32
            if p == 0 and (s * 32) % tile == 0:
                lane = 0                                      # first sample of a tile (and sample 0)
            if p == 1 and (s * 32 + 32) % tile == 0:
                lane = 31                                     # last sample of a tile
            m = s * 32 + lane
            if s == n_sub - 1 and (p == 1 or m >= M):
                m = M - 1
            probes.append(m)
        passes.append(probes)
    runs = []
    for probes in passes:
        for i in range(0, len(probes), max_probes):
            runs.append(probes[i: i + max_probes])
    return runs
