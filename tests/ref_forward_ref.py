"""The Ref-NeRF counterpart of tests/forward_ref.py: fp64 references with worst-case element-wise bounds for every stage of the fused
Ref-NeRF forward (`ref_kernel`, nerf_amd/csrc/mlp_kernels.hip), each stage against ITS OWN dumped inputs.  Plain helper module (no
fixtures): tests/test_gpu_ref_forward_layers.py feeds it what ops.ref_forward_train wrote (17 dump slots, mask records, aux (M, 16),
rgbo, normal) and the blob ops.pack_weights wrote; tests/test_ref_forward_ref_host.py feeds it an honest CPU emulation and eleven planted
faults.  The blob (RefLayout: 18 layers, segment kind 'ide', the IDE table behind the bias table) is read by forward_ref.unpack.

THE DUMP (mlp_layout.h, ref_kernel).  17 slots of the geometry of forward_ref.geometry -- mlp_launch_ref_train instantiates the bf16
training forward on the 8-wave x 32-sample tile (256 samples) and the fp32 one on 4 waves x 32 (128): forward_ref.TILE; slots 0..7 = the spatial hidden layers,
9..16 = the directional ones, slot 8 = 15 K groups: 0..7 the bottle-neck vector INCLUDING its noise (feature f = row f of bottle_neck:
the D map), 8..10 the 39 computed directional inputs in IDE slot order (slot q = 8 (kg - 8) + e of lane half h: real part of term q for
h = 0, imaginary part for h = 1, q = 19 / h = 0: n.d, everything else zero: forward_ref.ide_slot_column), 11..14 the PE10 slot of the
position (backward_ref.pe_slot_column).  Read as rows (ops.train_dump_rows, 240 features) feature f is slot backward_ref.feature_slot(f).
The mask records follow the 17 slots; slot 8's are never written and never read here.  aux (M, 16) fp32: the pre-activation head rows
(normal 0..2, roughness 3, diffuse 4..6, density 7, tint 8..10), the spec pre-activations 11..13, zeros 14..15.

THE MATRIX STAGES (STAGES) go through forward_ref.check_stage with K = 16 NKG and the bounds derived there (hidden_tol / linear_tol);
the head rows and the spec rows are fp32 accumulators stored as they are (linear, both precisions); the bottle-neck is the new kind
'noisy' = round(s + noise) without ReLU (forward_ref.noisy_tol: the linear bound, one fp32 addition, in bf16 the half-ulp conversion).

THE ELEMENT-WISE STAGES.  u = 2^-24.  The kernel is built with -ffp-contract=off and without fast-math, so every operator of its source
is one separately rounded fp32 operation (an explicit fmaf is one rounding).  Each bound is a running error analysis of the kernel's
own expression tree, evaluated in fp64 per element next to the reference value (value, error) -> (value, error):
    product  fl(a^ b^):      |a| eb + |b| ea + ea eb + u (|a| + ea)(|b| + eb) + 2^-126        (one rounding of the computed product)
    sum      fl(a^ + b^):    ea + eb + u (|a| + ea + |b| + eb)      <- the rounding is charged to the ABSOLUTE-VALUE evaluation of the
                             sum, so cancelling sums (the IDE polynomial sum_k mat[k] z^k, the power recurrences of (x + i y)^m,
                             d - 2 (n.d) n) are bounded by sum |terms|, never by their small result
    fmaf     fl(a^ b^ + c^): the two above with ONE rounding
    quotient fl(a^ / b^):    (|a| + ea) / (|b| - eb) - |a| / |b| + 5 u q      2.5 ulp: the OpenCL full-profile figure the device library
                             documents for division (forward_ref cites the same source; hipcc's default is correctly rounded, 0.5 ulp)
    expf 3 ulp = 6 u, log1pf 2 ulp = 4 u, sqrtf 3 ulp = 6 u, powf 16 ulp = 32 u  (same table); an argument error ea of expf enters as
                             the factor e^ea - 1: the conditioning of exp(-sigma_l roughness) is in the formula (sigma_l up to 36)
    sigmoid 1 / (1 + expf(-z)):  ez / 4 + 8 u      (forward_ref's derivation)
  normal = -n / (|n| + 1e-7):  |n| = sqrtf((x x + y y) + z z): three products and two sums of non-negative terms, the square root halves
      the relative error of its argument and adds its own 6 u, the addition of fl32(1e-7) rounds once.  The reference is evaluated in fp64
      WITH the fp32 constant, so for |n| -> 0 the quotient stays conditioned by the constant (relative bound ~ 15 u for every |n|); a
      missing 1e-7 is a relative error of 1e-7 / |n|.
  roughness = softplus(rho - 1) (one rounded subtraction, expf, log1pf; beyond the threshold 20 the kernel returns its argument, which
      differs from softplus by < e^-x: added to the bound), reflection r = d - (2 (d.n)) n, n.d = (dx nx + dy ny) + dz nz on the kernel's
      own rounded normal -- none of them is dumped; their (value, error) pairs feed the IDE:
  IDE term t = (m, l):  ((re|im)[m] * poly_t) * att_l,  zp[k] = zp[k-1] z,  re[k] = re[k-1] x - im[k-1] y,  im[k] = re[k-1] y + im[k-1] x,
      poly_t = fmaf chain over mat[k][t] zp[k],  att_l = expf(fl(-sigma_l roughness)),  sigma = (1, 3, 10, 36) for l = (1, 2, 4, 8).
      The three padding slots of K group 10, lane half 1's slot 19 (the imaginary twin of n.d) and lane half 1's padding must be EXACTLY 0.
  rgb:  sig(spec) sig(tint) + sig(diffuse), or srgb(sig(spec) sig(tint) + sig(fl(diffuse - fl32(log 3)))) with
      srgb(x) = x <= fl32(0.0031308) ? fl32(12.92) x : (211 powf(max(2^-23, x), fl32(5/12)) - 11) / 200;  the error of powf's argument goes
      through the function itself (evaluated at x +- ex), and where x is within ex of the knee both branches are admitted.
  position slot:  the fetched position is pts[:, :3], or its contraction x (2 - 1/|x|) / |x| for |x| > 1 (norm3, two quotients, a sum, a
      product: analysed like the normal; within the norm's error of |x| = 1 both branches are admitted).  fp32: sin_quadrant(2^f x, h):
      the power of two is exact, the three-FMA Cody-Waite reduction rounds at most three times at <= 2^-25 each (|r| < 1): 1.5 u; sin
      polynomial: final fmaf u |s| <= 0.71 u, the cubic term (|r|^3 / 6 <= 0.081, relative error 4 u) 0.33 u: 2.6 u; cos polynomial: inner
      fmaf u, its z error 0.31 u, the quartic term 0.06 u, final fmaf u: 3.9 u.  Bound 4 u + 2^f ex.  bf16: octave 0 like fp32, the octaves
      above by angle doubling  s' = fl(fl(2 s) c),  c' = fmaf(-2 s, s, 1),  bounded by running the SAME recurrence on the error pair
      (Es, Ec) next to the exact (sin, cos): Es' = 2 (|c| Es + |s| Ec + Es Ec) + u..., Ec' = 4 |s| Es + 2 Es^2 + u....  A FINDING of this
      derivation: treated as independent worst cases the pair grows by up to 4 per octave (about 2.6 on average: ~1e-3 at octave 9),
      where the kernel's comment expects a factor 2 (the angular part); the rigorous bound is therefore comparable to the bf16 half ulp
      at the top octaves instead of far below it.  It still is a bound, and wrong octaves / swapped sin and cos / wrong components are
      errors of order 1.
  bf16 outputs (IDE, n.d, PE slots) add the half-ulp conversion of the computed value: 2^-8 (|v| + e).

Exact stages (limit 0 violations): mask records of slots 0..7 and 9..16 == [dumped activation > 0]; aux[:, 14:16] == 0;
rgbo[:, 3] == aux[:, 7] bit for bit.

None of these is fitted to what the kernel produces."""
import torch

import backward_ref as R
import forward_ref as F

U, TINY, HALF = F.U24, F.TINY, F.BF16_HALF_ULP
LAY = F.LAYOUTS["ref"]
N_SLOTS = F.DUMP_SLOTS["ref"]
HIDDEN_SLOTS = tuple(range(8)) + tuple(range(9, 17))
SLOT8_WIDTH = 240                                                  # 15 K groups
DIV_C, EXP_C, LOG1P_C, SQRT_C, POW_C = 5.0, 6.0, 4.0, 6.0, 32.0   # in units of u: 2.5, 3, 2, 3, 16 ulp
PE_C32 = 4.0
SIGMA = {1: 1.0, 2: 3.0, 4: 10.0, 8: 36.0}                         # l (l + 1) / 2
TM = (0, 1, 0, 1, 2, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6, 7, 8)
TL = (1, 1, 2, 2, 2, 4, 4, 4, 4, 4, 8, 8, 8, 8, 8, 8, 8, 8, 8)
EXACT = ("mask", "auxpad", "density")                              # stages that count violations: limit 0


def f32c(x):
    """a source-code constant as the fp32 value the compiler stores, widened"""
    return float(torch.tensor(x, dtype=torch.float32).double())


C_1E7, C_LOG3, C_KNEE, C_1292, C_P = f32c(1e-7), f32c(1.0986122886681098), f32c(0.0031308), f32c(12.92), f32c(0.4166666666666667)
C_EPS = 2.0 ** -23
REF_SRGB = 1

# ------------------------------------------------------------------------------------------------ slot 8
IDE_COL = [F.ide_slot_column(8 * (R.feature_slot(f)[0] - 8) + R.feature_slot(f)[2], R.feature_slot(f)[1]) for f in range(128, 176)]
PE_COL = [R.pe_slot_column(8 * (R.feature_slot(f)[0] - 11) + R.feature_slot(f)[2], R.feature_slot(f)[1], 10) for f in range(176, 240)]


def _scatter(rows, cols, width):
    used = [i for i, c in enumerate(cols) if c >= 0]
    assert sorted(cols[i] for i in used) == list(range(width)), "the slot map is not a bijection onto the reference's columns"
    out = rows.new_zeros((rows.shape[0], width))
    out[:, [cols[i] for i in used]] = rows[:, used]
    return out


def split_slot8(s8):
    """slot 8 rows (M, 240) -> (bottle-neck (M, 128), the 39 directional inputs [real 19 | imag 19 | n.d], [x | PE10(x)] (M, 63)) in the
    reference's column order.  The padding features are NOT dropped silently: check_dir_inputs / check_position compare them with 0."""
    return s8[:, :128], _scatter(s8[:, 128:176], IDE_COL, 39), _scatter(s8[:, 176:240], PE_COL, 63)


def join_slot8(bn, ide39, ex):
    """the inverse (host emulation): reference-order columns -> slot-order rows with zero padding"""
    out = bn.new_zeros((bn.shape[0], SLOT8_WIDTH))
    out[:, :128] = bn
    for i, c in enumerate(IDE_COL):
        if c >= 0:
            out[:, 128 + i] = ide39[:, c]
    for i, c in enumerate(PE_COL):
        if c >= 0:
            out[:, 176 + i] = ex[:, c]
    return out


# ------------------------------------------------------------------------------------------------ matrix stages
# (name, stream layer, rows of the layer, kind, inputs: dump slots / 'pe' / 'bn' / 'ide' concatenated in the reference's column order,
#  output: dump slot, 'bn' or columns of aux)
_ALL = slice(None)
STAGES = (
    [("S0", 0, _ALL, "hidden", ("pe",), 0)] + [("S%d" % i, i, _ALL, "hidden", (i - 1,), i) for i in (1, 2, 3)] +
    [("S4", 4, _ALL, "hidden", ("pe", 3), 4)] + [("S%d" % i, i, _ALL, "hidden", (i - 1,), i) for i in (5, 6, 7)] +
    [("bottleneck", 8, slice(0, 128), "noisy", (7,), "bn"), ("heads", 8, slice(128, 139), "linear", (7,), slice(0, 11))] +
    [("D0", 9, _ALL, "hidden", ("bn", "ide"), 9)] + [("D%d" % i, 9 + i, _ALL, "hidden", (8 + i,), 9 + i) for i in (1, 2, 3)] +
    [("D4", 13, _ALL, "hidden", ("bn", "ide", 12), 13)] + [("D%d" % i, 9 + i, _ALL, "hidden", (8 + i,), 9 + i) for i in (5, 6, 7)] +
    [("spec", 17, _ALL, "linear", (16,), slice(11, 14))])
F.STAGES["ref"] = STAGES
ELEMENTWISE = ("normal", "ide", "ndot", "rgb", "position")


def stage_input(ins, acts, bn, ide39, ex):
    return torch.cat([ex if i == "pe" else (bn if i == "bn" else (ide39 if i == "ide" else acts[i])) for i in ins], dim=1)


# ------------------------------------------------------------------------------------------------ running error analysis
def _mul(a, ea, b, eb):
    m = (a.abs() + ea) * (b.abs() + eb)
    return a * b, a.abs() * eb + b.abs() * ea + ea * eb + U * m + TINY


def _add(a, ea, b, eb):
    return a + b, ea + eb + U * (a.abs() + ea + b.abs() + eb)


def _fma(a, ea, b, eb, c, ec):
    m = (a.abs() + ea) * (b.abs() + eb)
    return a * b + c, a.abs() * eb + b.abs() * ea + ea * eb + ec + U * (m + c.abs() + ec) + TINY


def _div(a, ea, b, eb):
    lo = (b.abs() - eb).clamp_min(TINY)
    q = (a.abs() + ea) / lo
    return a / b, (q - a.abs() / b.abs()) + DIV_C * U * q + TINY


def _exp(a, ea):
    v = torch.exp(a)
    return v, v * (torch.expm1(ea) + EXP_C * U * torch.exp(ea)) + TINY


def _sigmoid(a, ea):
    return torch.sigmoid(a), ea / 4 + F.SIGMOID_C * U


def _sqrt(a, ea):
    hi = torch.sqrt(a + ea)
    return torch.sqrt(a), (hi - torch.sqrt(a)) + SQRT_C * U * hi


def _zero(a):
    return torch.zeros_like(a)


def _norm3(x, y, z):
    o = _zero(x)
    s = _add(*_add(*_mul(x, o, x, o), *_mul(y, o, y, o)), *_mul(z, o, z, o))
    return _sqrt(*s)


def _softplus(x, ex):
    v = torch.logaddexp(x, _zero(x))
    t = torch.sigmoid(x + ex)                                       # e^x / (1 + e^x): what an error of e^x costs behind log1p
    return v, ex + EXP_C * U * t * torch.exp(ex) + LOG1P_C * U * (v + ex + EXP_C * U) + torch.where(x > 19.0, torch.exp(-x), _zero(x)) + TINY


def _report(got, want, tol):
    g = got.double()
    diff = (g - want).abs()
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / tol)              # (tol == 0: an element that must be exact)
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    k = int(ratio.reshape(-1).argmax())
    n = ratio.shape[1]
    return {"worst": float(ratio.reshape(-1)[k]), "where": (k // n, k % n), "neg_nonzero": 0}


def _stored(v, e, prec):
    """the bound of a value written into a B-operand slot: bf16 adds the half-ulp conversion of the computed value"""
    return e + HALF * (v.abs() + e) if prec == "bf16" else e


def normal_ref(aux):
    """-> ((value, error) of the three components of -n / (|n| + 1e-7), (value, error) of |n| + 1e-7)"""
    n = aux[:, 0:3].double()
    nn = _add(*_norm3(n[:, 0], n[:, 1], n[:, 2]), torch.full_like(n[:, 0], C_1E7), _zero(n[:, 0]))
    return [_div(-n[:, c], _zero(n[:, c]), *nn) for c in range(3)], nn


def check_normal(aux, normal):
    comp, _ = normal_ref(aux)
    return _report(normal, torch.stack([v for v, _ in comp], 1), torch.stack([e for _, e in comp], 1))


def dir_state(aux, dirs):
    """(value, error) pairs of everything between the head rows and the IDE terms, as ref_kernel forms it -- and as ref_heads_delta_kernel
    (bwd_kernels.hip) re-forms it with the same expressions: -> dict comp (3 pairs: the normal), nn (|n0| + 1e-7), dot (n.d), r (3 pairs: the
    reflection), rough, zp / re / im (9 pairs each: z^k, Re / Im (x + i y)^k), att {l: pair}"""
    comp, nn = normal_ref(aux)
    d = dirs.double()
    o = _zero(d[:, 0])
    dot = _add(*_add(*_mul(d[:, 0], o, *comp[0]), *_mul(d[:, 1], o, *comp[1])), *_mul(d[:, 2], o, *comp[2]))
    t2 = (2.0 * dot[0], 2.0 * dot[1])
    r = []
    for c in range(3):
        p = _mul(*t2, *comp[c])
        r.append(_add(d[:, c], o, -p[0], p[1]))
    rough = _softplus(*_add(aux[:, 3].double(), o, torch.full_like(o, -1.0), o))
    (x, ex), (y, ey), (z, ez) = r
    one = torch.ones_like(o)
    zp, re, im = [(one, o)], [(one, o)], [(o, o)]
    for k in range(1, 9):
        zp.append((zp[0][0] * z, ez) if k == 1 else _mul(*zp[k - 1], z, ez))
        a, b = _mul(*re[k - 1], x, ex), _mul(*im[k - 1], y, ey)
        re.append(_add(a[0], a[1], -b[0], b[1]))
        a, b = _mul(*re[k - 1], y, ey), _mul(*im[k - 1], x, ex)
        im.append(_add(*a, *b))
    att = {l: _exp(*_mul(torch.full_like(o, -sg), o, *rough)) for l, sg in SIGMA.items()}
    return {"comp": comp, "nn": nn, "dot": dot, "r": r, "rough": rough, "zp": zp, "re": re, "im": im, "att": att}


def dir_inputs_ref(aux, dirs, table):
    """fp64 (value, error) of the 39 computed directional inputs in the reference's column order [real 19 | imag 19 | n.d], from the
    kernel's own head values and the directions as fetch_sample hands them over (raw, not normalised).  table = the (9, 19) IDE table."""
    st = dir_state(aux, dirs)
    dot, zp, re, im, att = st["dot"], st["zp"], st["re"], st["im"], st["att"]
    o = _zero(dot[0])
    mat = table.double()
    real, imag = [], []
    for t in range(19):
        m, l = TM[t], TL[t]
        poly = (o, o)
        for k in range(l - m + 1):
            poly = _fma(mat[k, t].expand_as(o), o, *zp[k], *poly)
        real.append(_mul(*_mul(*re[m], *poly), *att[l]))
        imag.append(_mul(*_mul(*im[m], *poly), *att[l]))
    cols = real + imag + [dot]
    return torch.stack([v for v, _ in cols], 1), torch.stack([e for _, e in cols], 1)


def check_dir_inputs(aux, dirs, table, s8, prec):
    """slot 8 K groups 8..10 (all 48 features, padding included) -> {'ide': report over the 38 IDE values and the 9 zero slots,
    'ndot': report of the n.d slot}; where = (sample, feature 128.. of slot 8)"""
    want, err = dir_inputs_ref(aux, dirs, table)
    tol = _stored(want, err, prec)
    got = s8[:, 128:176].double()
    w48, t48 = got.new_zeros(got.shape), got.new_zeros(got.shape)
    for i, c in enumerate(IDE_COL):
        if c >= 0:
            w48[:, i], t48[:, i] = want[:, c], tol[:, c]
    i_dot = IDE_COL.index(38)
    rest = [i for i in range(48) if i != i_dot]
    ide = _report(got[:, rest], w48[:, rest], t48[:, rest])
    ide["where"] = (ide["where"][0], 128 + rest[ide["where"][1]])
    nd = _report(got[:, [i_dot]], w48[:, [i_dot]], t48[:, [i_dot]])
    nd["where"] = (nd["where"][0], 128 + i_dot)
    return {"ide": ide, "ndot": nd}


def srgb_ref(x, ex):
    o = _zero(x)
    s0 = _mul(torch.full_like(x, C_1292), o, x, ex)
    m = x.clamp_min(C_EPS)
    p = m ** C_P
    hi, lo = (m + ex) ** C_P, (m - ex).clamp_min(C_EPS) ** C_P
    ep = torch.maximum(hi - p, p - lo) + POW_C * U * hi
    s1 = _div(*_add(*_mul(torch.full_like(x, 211.0), o, p, ep), torch.full_like(x, -11.0), o), torch.full_like(x, 200.0), o)
    below = x <= C_KNEE
    want, tol = torch.where(below, s0[0], s1[0]), torch.where(below, s0[1], s1[1])
    near = (x - C_KNEE).abs() <= ex
    return want, torch.where(near, torch.maximum(s0[1], s1[1]) + (s0[0] - s1[0]).abs(), tol)


def rgb_ref(aux, flags):
    a = aux.double()
    want, tol = [], []
    for c in range(3):
        o = _zero(a[:, 0])
        spec, tint, dif = a[:, 11 + c], a[:, 8 + c], a[:, 4 + c]
        dd = _add(dif, o, torch.full_like(o, -C_LOG3), o) if flags & REF_SRGB else (dif, o)
        lin = _add(*_mul(*_sigmoid(spec, o), *_sigmoid(tint, o)), *_sigmoid(*dd))
        w, t = srgb_ref(*lin) if flags & REF_SRGB else lin
        want.append(w)
        tol.append(t)
    return torch.stack(want, 1), torch.stack(tol, 1)


def check_rgb(aux, rgbo, flags):
    want, tol = rgb_ref(aux, flags)
    return _report(rgbo[:, :3], want, tol)


def position_ref(pts, contract):
    """fp64 (value, error) of the position fetch_sample hands to the encoder: pts[:, :3], contracted for |x| > 1 when the flag is set"""
    x = pts[:, :3].double()
    o = _zero(x)
    if not contract:
        return x, o
    n, en = _norm3(x[:, 0], x[:, 1], x[:, 2])
    oo, one = _zero(n), torch.ones_like(n)
    outside, edge = n > 1.0, (n - 1.0).abs() <= en
    ns, ens = n.clamp_min(1.0), torch.where(outside | edge, en, oo)
    inv = _div(one, oo, ns, ens)
    k, ek = _div(*_add(2.0 * one, oo, -inv[0], inv[1]), ns, ens)                    # (2 - 1 / n) / n
    ek = torch.where(edge, ek + (k - 1.0).abs(), ek)                               # either branch is admitted at the boundary
    v, e = _mul(x, o, k[:, None].expand_as(x), ek[:, None].expand_as(x))
    return torch.where(outside[:, None], v, x), torch.where((outside | edge)[:, None], e, o)


def position_slot_ref(pts, contract, prec):
    """fp64 (value, tolerance) of [x | PE10(x)] (M, 63) in the reference's column order [x y z | sin f0 xyz | cos f0 xyz | ...]"""
    x, ex = position_ref(pts, contract)
    want, tol = [x], [_stored(x, ex, prec)]
    if prec == "fp32":
        for f in range(10):
            a = x * 2.0 ** f
            e = PE_C32 * U + 2.0 ** f * ex
            want += [torch.sin(a), torch.cos(a)]
            tol += [e, e]
    else:
        s, c = torch.sin(x), torch.cos(x)
        es = ec = PE_C32 * U + ex
        for f in range(10):
            want += [s, c]
            tol += [_stored(s, es, prec), _stored(c, ec, prec)]
            s2 = (2.0 * s, 2.0 * es)
            ns = _mul(*s2, c, ec)
            nc = _fma(-s2[0], s2[1], s, es, torch.ones_like(s), _zero(s))
            (s, es), (c, ec) = ns, nc
    return torch.cat(want, 1), torch.cat(tol, 1)


def check_position(pts, contract, s8, prec):
    """slot 8 K groups 11..14 (all 64 features: the zero padding too); where = (sample, feature 176.. of slot 8)"""
    want, tol = position_slot_ref(pts, contract, prec)
    got = s8[:, 176:240].double()
    w64, t64 = got.new_zeros(got.shape), got.new_zeros(got.shape)
    for i, c in enumerate(PE_COL):
        if c >= 0:
            w64[:, i], t64[:, i] = want[:, c], tol[:, c]
    rep = _report(got, w64, t64)
    rep["where"] = (rep["where"][0], 176 + rep["where"][1])
    return rep


def _count(bad):
    n = int(bad.sum())
    first = None
    if n:
        k = int(bad.reshape(-1).float().argmax())
        first = (k // bad.shape[1], k % bad.shape[1])
    return {"worst": float(n), "where": first, "neg_nonzero": 0}


# ------------------------------------------------------------------------------------------------ everything
def check_forward(prec, u, run, pts, noise, flags, contract=False):
    """Every stage of one training forward.  run: acts {slot: rows} for HIDDEN_SLOTS, s8 (M, 240), aux (M, 16), rgbo (M, 4), normal (M, 3),
    optionally masks {slot: bool rows}; u = the unpacked blob (forward_ref.unpack, with u.ide); pts (M, 6) as given to the kernel;
    noise (M, 128) or None.  -> {stage: report}"""
    acts, s8, aux = run["acts"], run["s8"], run["aux"]
    bn, ide39, ex = split_slot8(s8)
    rep = {}
    for name, l, rows, kind, ins, dst in STAGES:
        x = stage_input(ins, acts, bn, ide39, ex)
        got = acts[dst] if kind == "hidden" else (bn if kind == "noisy" else aux[:, dst])
        rep[name] = F.check_stage(got, x, u.w[l][rows], u.b[l][rows], 16 * LAY.NKG[l], prec, kind, add=noise if kind == "noisy" else None)
    rep["normal"] = check_normal(aux, run["normal"])
    rep.update(check_dir_inputs(aux, pts[:, 3:6], u.ide, s8, prec))
    rep["rgb"] = check_rgb(aux, run["rgbo"], flags)
    rep["position"] = check_position(pts, contract, s8, prec)
    rep["auxpad"] = _count(aux[:, 14:16] != 0)
    rep["density"] = _count((run["rgbo"][:, 3].contiguous().view(torch.int32) != aux[:, 7].contiguous().view(torch.int32))[:, None])
    if run.get("masks") is not None:
        bad, first = 0, None
        for L in HIDDEN_SLOTS:
            diff = run["masks"][L] != (acts[L] > 0)
            n = int(diff.sum())
            if n and first is None:
                k = int(diff.reshape(-1).float().argmax())
                first = (L, k // diff.shape[1], k % diff.shape[1])
            bad += n
        rep["mask"] = {"worst": float(bad), "where": first, "neg_nonzero": 0}
    return rep


def limit(stage):
    return 0.0 if stage in EXACT else 1.0


def ratios(rep):
    return F.ratios(rep)


def failing(rep):
    return sorted(k for k, v in F.ratios(rep).items() if not v <= limit(k))


def assert_forward(what, rep):
    bad = failing(rep)
    assert not bad, "%s: beyond the bound in %s" % (what, ", ".join(
        "%s (%.3g at %s, %d not zero where s < -tol)" % (k, rep[k]["worst"], rep[k]["where"], rep[k]["neg_nonzero"]) for k in bad))


# ------------------------------------------------------------------------------------------------ masters
def kernel_tensors(sd, table):
    """a RefNeRF state_dict -> the 20 weights / 20 biases pack_ref takes (RefNeRF._pack_tensors): spatial 0..7, bottle_neck 8, the 11 head
    rows in kernel order 9, directional 10..17, spec head 18, the IDE table 19 (its bias slot repeats the head bias: never read)"""
    nw, nb, rw, rb = sd["norm_col_tint_head.weight"], sd["norm_col_tint_head.bias"], sd["rho_tau_head.weight"], sd["rho_tau_head.bias"]
    hw = torch.cat((nw[0:3], rw[0:1], nw[3:6], rw[1:2], nw[6:9]), 0).contiguous()
    hb = torch.cat((nb[0:3], rb[0:1], nb[3:6], rb[1:2], nb[6:9]), 0).contiguous()
    names = ["spa_block1.%d" % i for i in (0, 2, 4, 6)] + ["spa_block2.%d" % i for i in (0, 2, 4, 6)] + ["bottle_neck"]
    tail = ["dir_block1.%d" % i for i in (0, 2, 4, 6)] + ["dir_block2.%d" % i for i in (0, 2, 4, 6)] + ["spec_rgb_head.0"]
    ws = [sd[n + ".weight"] for n in names] + [hw] + [sd[n + ".weight"] for n in tail] + [table]
    bs = [sd[n + ".bias"] for n in names] + [hb] + [sd[n + ".bias"] for n in tail] + [hb]
    return [w.detach().float().contiguous() for w in ws], [b.detach().float().contiguous() for b in bs]


UNITS7 = (103, 228, 6, 15, 255, 221, 193, 44)          # units of the last spatial / directional layer (he weights) that are switched on for
UNITS16 = (169, 237, 39, 95, 144, 20)                                # about half of the samples: found with `emulate`, re-checked by the host test


def varied_state():
    """The third weight set: he weights whose heads VARY, so that the element-wise stages are exercised over their whole range.  A head
    row gets, on top of its he row, c (e_j - e_k) for two hidden units j, k that are each on for about half of the samples: the
    pre-activation then takes both signs with a spread of several units whatever the rest of the row does.
      roughness (c = 8): exp(-36 softplus(rho - 1)) underflows for some samples and stays near 1 for others;
      diffuse, tint, spec (c = 4): both signs in every channel;
      normal rows: ZERO but for one unit (weights (6, -3.2, 2.4)) and biases of (2, -1, 3) e-7: a sample with that unit switched off
        has |n| = |bias| ~ 3.7e-7, where the 1e-7 of the normalisation carries a fifth of the quotient; a sample with it on has |n| up
        to several units."""
    import weights as W
    sd = {k: v.clone() for k, v in W.ref_state("he").items()}

    def spread(row, units, i, c):
        row[units[i % len(units)]] += c
        row[units[(i + 3) % len(units)]] -= c
    spread(sd["rho_tau_head.weight"][0], UNITS7, 0, 8.0)
    nw, nb = sd["norm_col_tint_head.weight"], sd["norm_col_tint_head.bias"]
    nw[0:3] = 0.0
    nw[0:3, UNITS7[0]] = torch.tensor([6.0, -3.2, 2.4])
    nb[0:3] = torch.tensor([2e-7, -1e-7, 3e-7])
    for r in range(3, 9):
        spread(nw[r], UNITS7, r - 2, 4.0)
    for r in range(3):
        spread(sd["spec_rgb_head.0.weight"][r], UNITS16, r, 4.0)
    return sd


def coverage(aux):
    """the conditions the varied set has to meet on the dumped aux -> dict of booleans (all must hold)"""
    a = aux.double()
    att8 = torch.exp(-36.0 * torch.nn.functional.softplus(a[:, 3] - 1.0))
    n = a[:, 0:3].norm(dim=1)
    out = {"att8 < 1e-30": bool((att8 < 1e-30).any()), "att8 > 0.5": bool((att8 > 0.5).any()),
           "|n| < 1e-3": bool((n < 1e-3).any()), "|n| > 1": bool((n > 1.0).any())}
    for name, c0 in (("diffuse", 4), ("tint", 8), ("spec", 11)):
        for c in range(3):
            out["%s %d both signs" % (name, c)] = bool((a[:, c0 + c] > 0).any()) and bool((a[:, c0 + c] < 0).any())
    return out


# ------------------------------------------------------------------------------------------------ honest emulation (host test, set choice)
def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _fma32(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def ide_f32(x, y, z, rough, table, fault=None):
    """ide_encode in fp32, operation by operation -> (real (M, 19), imag (M, 19))"""
    one = torch.ones_like(x)
    zp, re, im = [one], [one], [torch.zeros_like(x)]
    for k in range(1, 9):
        zp.append(zp[k - 1] * z)
        re.append(re[k - 1] * x - im[k - 1] * y)
        im.append(re[k - 1] * y + im[k - 1] * x)
    sig = dict(SIGMA)
    if fault == "sigma4":
        sig[4] = 6.0
    att = {l: torch.exp(-s * rough) for l, s in sig.items()}
    real, imag = [], []
    for t in range(19):
        m, l = TM[t], TL[t]
        poly = torch.zeros_like(x)
        for k in range(l - m + 1):
            poly = _fma32(table[k, t].expand_as(x), zp[k], poly)
        real.append((re[m] * poly) * att[l])
        imag.append((im[m] * poly) * att[l])
    if fault == "reim":
        real[7], imag[7] = imag[7], real[7]
    return torch.stack(real, 1), torch.stack(imag, 1)


def srgb_f32(x):
    s0 = torch.tensor(12.92, dtype=torch.float32) * x
    s1 = (211.0 * torch.maximum(torch.tensor(C_EPS, dtype=torch.float32), x) ** torch.tensor(0.4166666666666667, dtype=torch.float32) - 11.0) / 200.0
    return torch.where(x <= torch.tensor(0.0031308, dtype=torch.float32), s0, s1)


def emulate(prec, u, pts, noise=None, flags=0, contract=False, fault=None, at=None):
    """ref_kernel's arithmetic on the CPU, honestly: fp32 chains (torch's order), one round-to-nearest conversion per stored element, the
    element-wise expressions operation by operation in fp32.  fault / at: a planted fault (tests/test_ref_forward_ref_host.py) and where."""
    import torch_spec as T
    cast = lambda v: R.element(v, prec)
    pts = pts.float()
    M = pts.shape[0]
    pos = T.contract_expr(pts[:, :3]) if contract else pts[:, :3]
    d = pts[:, 3:6]
    ex = cast(torch.cat((pos, T._pe(pos, 10)), -1))
    acts, aux = {}, torch.zeros(M, 16)
    bn = ide39 = None
    zero = torch.zeros(M, 128) if noise is None else noise.float()
    for name, l, rows, kind, ins, dst in STAGES:
        if name == "D0":                                                            # the element-wise stage between the two networks
            n0 = aux[:, 0:3]
            rough = torch.nn.functional.softplus(aux[:, 3] - 1.0)
            nn = torch.sqrt((n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1]) + n0[:, 2] * n0[:, 2])
            if fault != "no1e-7":
                nn = nn + torch.tensor(1e-7)
            nrm = -n0 / nn[:, None]
            dot = (d[:, 0] * nrm[:, 0] + d[:, 1] * nrm[:, 1]) + d[:, 2] * nrm[:, 2]
            r = d - (2.0 * dot)[:, None] * nrm
            real, imag = ide_f32(r[:, 0], r[:, 1], r[:, 2], rough, u.ide, fault)
            ide39 = cast(torch.cat((real, imag, dot[:, None]), 1))
        x = stage_input(ins, acts, bn, ide39, ex).float()
        if fault == "stale" and name == at:                                         # K group 2 of D4's input read from another tile's stash
            x = x.clone()
            x[:, 32:48] = torch.roll(x[:, 32:48], 32, dims=0)
        w, b = u.w[l][rows].float(), u.b[l][rows].float()
        z = x @ w.t() + b
        if kind == "hidden":
            acts[dst] = (_trunc_bf16 if (fault == "trunc" and name == at) else cast)(torch.relu(z))
        elif kind == "noisy":
            nz = zero
            if fault == "noiseswap":
                nz = zero[:, [f ^ 8 if f // 16 == 3 else f for f in range(128)]]    # the two 4-feature runs of K group 3 trade places
            bn = cast(z + nz)
        else:
            aux[:, dst] = z
    if fault == "rows":                                                             # diffuse and tint rows exchanged
        aux[:, 4:7], aux[:, 8:11] = aux[:, 8:11].clone(), aux[:, 4:7].clone()
    sig = torch.sigmoid
    use_srgb = bool(flags & REF_SRGB) and fault != "nosrgb"
    if use_srgb:
        rgb = srgb_f32(sig(aux[:, 11:14]) * sig(aux[:, 8:11]) + sig(aux[:, 4:7] - torch.tensor(1.0986122886681098)))
    else:
        rgb = sig(aux[:, 11:14]) * sig(aux[:, 8:11]) + sig(aux[:, 4:7])
    rgbo = torch.cat((rgb, aux[:, (6 if fault == "density6" else 7):][:, :1]), 1)
    if fault == "ndot20":                                                           # n.d lands one slot further
        s8 = join_slot8(bn, torch.cat((ide39[:, :38], torch.zeros(M, 1).to(ide39.dtype)), 1), ex)
        q20 = [i for i in range(48) if R.feature_slot(128 + i) == (10, 0, 4)][0]
        s8[:, 128 + q20] = ide39[:, 38]
    else:
        s8 = join_slot8(bn, ide39, ex)
    masks = {L: acts[L] > 0 for L in HIDDEN_SLOTS}
    return {"acts": acts, "s8": s8, "aux": aux, "rgbo": rgbo, "normal": nrm, "masks": masks}
