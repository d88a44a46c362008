"""fp64 specifications and element-wise bounds for the element-wise stages of the layer-by-layer route (nerf_amd/generic_path.py;
kernels in nerf_amd/csrc/generic_ref_kernels.hip and generic_kernels.hip), one stage at a time.  Plain helper module (no fixtures):
tests/test_gpu_generic_stages.py feeds it what the kernels wrote, tests/test_generic_ref_host.py checks it on the CPU -- the
specifications against the oracle and torch.autograd, the bounds against a torch-fp32 evaluation, and that the bounds bite -- before
it is trusted as a yardstick.

Every function takes the kernel's OWN fp32 inputs and returns the fp64 value of every output element and a bound for every element.
No bound is a whole-tensor relative number; none is fitted to what a kernel produces.  u = 2^-24 is the fp32 unit roundoff.

Specifications
  directional stage   ref_model.py:80-92 (kinv = softplus(rho - 1), n = -n0 / (|n0| + 1e-7), w_r = d - 2 (d.n) n, [IDE(w_r, kinv) | n.d])
                      with oracle.ide_encode / oracle.ide_tables -- the reference's fp32 table, widened, exactly as the oracle does
  colour combination  ref_model.py:98-105 with oracle.linear_to_srgb
  PE adjoint          rows [x | sin 2^0 x | cos 2^0 x | sin 2^1 x | ...] (nerf_helper.py:38-48)
  adjoints            torch.autograd in fp64 of those forwards
The kernels hold four constants as fp32 literals (1e-7, log 3, 323/25, 5/12 and 7/12 of the sRGB curve): `Consts.KERNEL` hands the
specification the same fp32 values widened (they are inputs of the kernel like its tensors are; fl32(5/12) alone moves x^(5/12) by
up to 2.7 u at x = 2^-23), `Consts.EXACT` the oracle's doubles for the comparison with the oracle.

Allowances for device math functions: 2 ulp = 4 u each for expf, log1pf, sinf, cosf, powf.  The HIP math API documents each of them
at 1 ulp maximum error; 1 ulp is at most 2 u relative (just above a power of two), and the documented figure is doubled because it
comes from testing, not from proof.  sqrtf and the division are taken as correctly rounded within 1 ulp (2 u): SQRT_U = DIV_U = 2.
  sigmoid 1 / (1 + expf(-v)):   SIG_U = 7   = 4 (expf, times e / (1 + e) <= 1) + 1 (the addition) + 2 (the division)
  softplus log1pf(expf(v)):     SP_U  = 8   = 4 (expf, times e / ((1 + e) log1p e) <= 1) + 4 (log1pf), on top of the rounding of
                                v = rho - 1, which moves kinv by at most u |v| sigmoid(v)

Directional stage, forward (dir_forward_check) -- the "own inputs" principle of backward_ref.py, in three steps:
  1. the predicted normal against -n0 / (|n0| + eps):  NORMAL_U = 8 = 3 (sum of three squares, relative: all terms positive) / 2 (the
     root halves it) + 2 (sqrtf) + 1 (+ eps) + 2 (division), rounded up from 6.5;  tol = 8 u |n_c|
  2. n.d against the fp64 dot product of the kernel's OWN normal with d:  three products and two additions, tol = 3 u sum_c |n_c d_c|
  3. IDE against ide(r*, kinv) (= oracle.ide_encode, see there) with r* = d - 2 (n.d) n formed in fp64 from the kernel's own normal and n.d outputs.
     With w = x + i y, P_t(z) = sum_k mat[k, t] z^k, |P|_t = sum_k |mat[k, t]| |z|^k, att_l = exp(-l (l + 1) / 2 kinv) and the
     magnitude A = att |w|^m |P|_t, real and imaginary part of term t = (l, m) each get
         tol = u A (4 m + 2 l + 2 + 4 + sig_l kinv (1 + SP_U) + sig_l |v| sigmoid(v))            sig_l = l (l + 1) / 2
               + 1.01 att (|w|^m sum_k k |mat| |z|^(k-1) dz + m |w|^(m-1) |P|_t (dx + dy))      the rounding of w_r, first order
               + 2^-126 (1 + |w|^m |P|_t)                                                       att or a product below the normal range
       4 m      (x + i y)^m by m - 1 complex multiplications, each within 2 sqrt(2) u of the modulus: 2.83 (m - 1) <= 4 m
       2 l      z^k by k - 1 multiplications, the l - m + 1 terms added by fused multiply-adds: (k - 1) + (l - m + 1) <= 2 l
       2        the two final products; 4 expf; sig_l kinv u the rounding of the exponent, sig_l times kinv's own error after it
       dx, dy, dz = 2.01 u (|d_c| + 2 |n.d| |n_c|): the kernel rounds 2 (n.d) n_c once (the doubling is exact) and the difference once.
     A carries the cancellation of the degree-16 polynomials: over dir_inputs(1000, 5) the median of |P|_t / |P_t| is 2e3 at (l, m) =
     (16, 0), its 90th percentile 2e5.

Directional stage, adjoint (dir_backward_spec): the fp64 value is torch.autograd of the forward specification w.r.t. head columns
0-2 and 9.  The bound is u (C A + A_att) + 2^-126 1e4 / (|n0| + eps):
  A      the magnitude pass of the adjoint (dir_backward_explicit(mag=True): the kernel's formula with every tensor replaced by its
         absolute value, every difference by a sum, every power of x + i y by the power of its modulus, at the true forward values)
  A_att  DERIVED: the adjoint is linear in the attenuations att_l, so the effect of their relative error att_depth(l) u = (4 + sig_l
         kinv (1 + SP_U) + sig_l |v| sigmoid(v)) u is the same pass with every att_l multiplied by att_depth(l); at kinv = 20 and
         l = 16 that is 2.4e4 u, far beyond any constant depth (without this term the measured C below ranged 7 .. 19)
  C      the adjoint also multiplies second derivatives of the polynomials by the few-u rounding of w_r, for which no depth was
         derived; C is MEASURED AGAINST THE REFERENCE, never against the kernel: the smallest C that holds a torch-fp32 CPU evaluation
         of the same specification (the explicit formula, and torch.autograd in fp32 of the forward) over the test's inputs
         (dir_inputs(M, deg), M in MS), times 4 (device math functions are specified to a few ulp where the host libm is within
         one; the compiler may contract multiply-adds):
              ide_level        1      2      3      4      5
              measured       3.85   3.80   2.83   2.94   3.91          (DIR_BWD_MEASURED)
         C = 16 = 4 x 3.91 rounded up, at every level (DIR_BWD_C).  test_generic_ref_host.py re-measures.
The last term covers a product below the normal range times the gains behind it (k |w|^(k-1) <= 300, 2 |n.d|, 1 / (|n0| + eps)).

Colour combination (combine_spec), lin = s sigmoid(tint) + sigmoid(diffuse [- log 3]), s = the spec head (an input):
  tol_lin = u ((SIG_U + 2) s st + (SIG_U + 1) sd) [+ u |diffuse - log 3| sd (1 - sd)]      product, sum; the shifted argument's rounding
  linear:       tol = tol_lin
  sRGB, below:  tol = 12.92 tol_lin + u |out|
  sRGB, above:  tol = (211 x^p (5 u + p tol_lin / lin) + u |211 x^p - 11|) / 200 + 2 u |out|       p = 5/12; 4 powf + 1 product
  density:      copied, tol = 0 (bit-equal).   Every row's lin must be further than tol_lin from the knee (asserted).
Its adjoint (combine_backward_spec; autograd of the above): with y (1 - y) of a sigmoid y known to eps_y formed as fl(y fl(1 - y)):
  e_q(y, eps_y) = y (eps_y |1 - 2 y| + 2 u (1 - y));   gl = g slope(lin):  eps_gl = u (1 [+ 4 powf + 3 constants] ) [+ 7/12 tol_lin / lin
  + |fl32(5/12) - 1 + fl32(7/12)| |ln lin|: the kernel's slope exponent is the literal fl32(7/12), 3e-8 off the derivative of its forward]
  d_spec = (gl st) (s (1 - s)):       tol = |ref| (eps_gl + (SIG_U + 4) u)
  d_diffuse = gl (sd (1 - sd)):       tol = |gl| e_q(sd, eps_sd) + |ref| (eps_gl + u)
  d_tint = (gl s) (st (1 - st)):      tol = |gl s| e_q(st, SIG_U u) + |ref| (eps_gl + 2 u)
  d_density: copied, tol = 0.

PE adjoint (pe_backward_spec): d_x[c] = d_enc[c] + sum_f 2^f (cos(a_f) d_sin[f, c] - sin(a_f) d_cos[f, c]), a_f = 2^f x32 exact in
both precisions.  tol = (L + 7) u (|d_enc[c]| + sum_f 2^f (|cos a_f d_sin| + |sin a_f d_cos|)): 4 (sinf / cosf) + 1 (product) + 1
(the difference) per term, the scaling by 2^f exact, L + 1 additions.

Scene contraction (contract_spec; oracle.contract and its autograd): forward 14 u |out| = 4 (norm: 1.5 + 2, rounded up) + 3 (1 / r
and 2 - 1 / r >= 1) + 6 (the second division by r, with r's own error) + 1 (product); pull-back 48 u A with A = k |g_c| + sum_i
|u_i g_i| (1 / r^2 + k) |u_c|: 14 (k) + 6 (u_c) + 9 (u.g) + 14 (1 / r^2 - k) + 5 (products, sum).  Value and Jacobian are continuous
at r = 1, so a computed radius on the other side of 1 than the exact one stays inside the bound.

Layer product (gemm_spec): (P + 2) u sum_p |a_ip b_pj| (+ |bias_j|), operands rounded to bf16 first in bf16 mode (their products
are then exact in fp32); the sigmoid adds SIG_U u sigmoid(v) and multiplies the sum's bound by sigmoid'(v); ReLU passes the bound.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import nerf_oracle as O  # noqa: E402

U = 2.0 ** -24
TINY = 2.0 ** -126
FN_U = 4.0            # expf, log1pf, sinf, cosf, powf: 2 ulp
SQRT_U = DIV_U = 2.0
SIG_U = 7.0
SP_U = 8.0
NORMAL_U = 8.0
CONTRACT_FWD_U, CONTRACT_BWD_U = 14.0, 48.0
KNEE = 0.0031308

# the smallest C that holds the torch-fp32 evaluations of the adjoint over dir_inputs(M, deg), M in MS (dir_backward_measure), and 4 x the
# largest of them, rounded up.  tests/test_generic_ref_host.py::test_dir_backward_constant_is_four_times_the_fp32_evaluation re-measures.
DIR_BWD_MEASURED = {1: 3.85, 2: 3.80, 3: 2.83, 4: 2.94, 5: 3.91}
DIR_BWD_C = {deg: 16.0 for deg in (1, 2, 3, 4, 5)}

MS = (1, 255, 256, 257, 1000)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


class Consts:
    def __init__(self, eps_n, log3, c1292, p512, p712, knee):
        self.eps_n, self.log3, self.c1292, self.p512, self.p712, self.knee = eps_n, log3, c1292, p512, p712, knee


Consts.EXACT = Consts(1e-7, math.log(3.), 323 / 25, 5 / 12, 7 / 12, KNEE)
Consts.KERNEL = Consts(f32(1e-7), f32(1.0986122886681098), f32(12.92), f32(5 / 12), f32(7 / 12), f32(KNEE))


# ------------------------------------------------------------------------------------------------ the comparator
def compare(got, ref, tol):
    """-> {"worst": max(err / tol) over EVERY element, "where": its index}: a non-finite element, or an error where tol == 0, is inf."""
    g, r, t = got.detach().double().cpu(), ref.detach().double().cpu(), tol.detach().double().cpu().expand_as(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if g.numel() == 0:
        return {"worst": 0.0, "where": ()}
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / t)              # x / 0 = inf
    ratio = torch.where(torch.isfinite(g) & torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    k = int(ratio.argmax())
    return {"worst": float(ratio.reshape(-1)[k]), "where": tuple(int(i) for i in torch.unravel_index(torch.tensor(k), ratio.shape))}


def worst(*reports):
    return max(r["worst"] for r in reports)


# ------------------------------------------------------------------------------------------------ inputs (fixed seeds)
def T_of(deg):
    return (1 << deg) - 1 + deg


def ide_terms(deg):
    """[(l, m)] in the table's column order, and the fp32 table widened (LMAX + 1, T)"""
    ml, mat = O.ide_tables(deg)
    return [(int(l), int(m)) for m, l in ml.t().tolist()], mat.double()


def dir_inputs(M, deg, seed=11):
    """-> heads (M, 11), dirs (M, 3), d_out (M, 2T + 1), g_normal (M, 3), spec (M, 3), g_rgbo (M, 4) fp32.  randn heads, the roughness
    column spread so that softplus(rho - 1) spans 1e-3 .. 20, |dirs| in 0.8 .. 1.2; from row 1 on (as many as fit) the hand-made rows:
    zero normal, |normal| = 1e-6, normal parallel / anti-parallel to the direction, w_r along +z / -z, roughness +30 / -30."""
    g = torch.Generator().manual_seed(seed + 100 * deg + M)
    T = T_of(deg)
    h = torch.randn(M, 11, generator=g)
    lo, hi = math.log(math.expm1(1e-3)) + 1.0, 21.0                      # softplus(rho - 1) = 1e-3 .. 20
    h[:, 9] = lo + (hi - lo) * torch.rand(M, generator=g)
    d = F.normalize(torch.randn(M, 3, generator=g), dim=-1) * (0.8 + 0.4 * torch.rand(M, 1, generator=g))
    hand = []
    zero = h[0].clone(); zero[0:3] = 0.0; hand.append((zero, d[0].clone()))
    tiny = h[0].clone(); tiny[0:3] = F.normalize(h[0, 0:3], dim=0) * 1e-6; hand.append((tiny, d[0].clone()))
    par = h[0].clone(); par[0:3] = d[0] * 1.7; hand.append((par, d[0].clone()))
    anti = h[0].clone(); anti[0:3] = -d[0] * 0.6; hand.append((anti, d[0].clone()))
    for s in (1.0, -1.0):                                                # n along x, d along z: n.d = 0, w_r = d = (0, 0, +-|d|)
        row = h[0].clone(); row[0:3] = torch.tensor([-1.3, 0.0, 0.0]); hand.append((row, torch.tensor([0.0, 0.0, 1.1 * s])))
    for rho in (30.0, -30.0):
        row = h[0].clone(); row[9] = rho; hand.append((row, d[0].clone()))
    for i, (hr, dr) in enumerate(hand):
        if 1 + i < M:
            h[1 + i], d[1 + i] = hr, dr
    return (h.contiguous(), d.contiguous(), torch.randn(M, 2 * T + 1, generator=g), torch.randn(M, 3, generator=g),
            torch.sigmoid(torch.randn(M, 3, generator=g) * 2), torch.randn(M, 4, generator=g))


def combine_inputs(M, srgb, seed=23):
    """heads, spec, g_rgbo; with srgb the first rows (as many as fit) are placed on both sides of the knee: lin = knee -+ 1e-4 .. by
    construction (tint very negative: spec * sigmoid(tint) ~ 0, diffuse chosen so that sigmoid(diffuse - log 3) = the wanted lin)."""
    g = torch.Generator().manual_seed(seed + M + (7 if srgb else 0))
    h = torch.randn(M, 11, generator=g) * 2
    s = torch.sigmoid(torch.randn(M, 3, generator=g) * 3)
    gr = torch.randn(M, 4, generator=g)
    if srgb:
        for i, lin in enumerate((KNEE - 1e-4, KNEE + 1e-4, KNEE - 2e-4, KNEE + 3e-4, 1e-3, 5e-3, 2e-4, 1e-5)):
            if i < M:
                h[i, 6:9] = -40.0
                h[i, 3:6] = math.log(lin / (1 - lin)) + math.log(3.)
                s[i] = torch.tensor([0.0, 0.5, 1.0])
    if M > 9:
        s[9] = torch.tensor([0.0, 1.0, 0.5]); h[9, 3:9] = torch.tensor([30.0, -30.0, 0.0, 30.0, -30.0, 0.0])
    return h.contiguous(), s.contiguous(), gr.contiguous()


def pe_inputs(M, L, cat_origin, seed=37):
    """x (M, 3): |x| <= 1.5, plus (when they fit) contracted-range rows (|x| up to 2) and rows with |x_c| = 8; d_enc (M, E) randn"""
    g = torch.Generator().manual_seed(seed + 1000 * L + M + int(cat_origin))
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * 1.5
    for i, row in enumerate(((1.9, -1.99, 2.0), (8.0, -8.0, 8.0), (0.0, -0.0, 1e-30), (-2.0, 1.75, -1.9))):
        if 2 + i < M:
            x[2 + i] = torch.tensor(row)
    E = 6 * L + (3 if cat_origin else 0)
    return x.contiguous(), torch.randn(M, E, generator=g)


def contract_inputs(M, seed=41):
    g = torch.Generator().manual_seed(seed + M)
    x = torch.randn(M, 3, generator=g) * torch.exp(torch.randn(M, 1, generator=g) * 1.5)
    one_up = float(torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)))
    for i, row in enumerate(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, one_up), (-one_up, 0.0, 0.0), (6e5, -8e5, 0.0),
                             (0.6, 0.8, 0.0))):
        if 1 + i < M:
            x[1 + i] = torch.tensor(row)
    return x.contiguous(), torch.randn(M, 3, generator=g)


# ------------------------------------------------------------------------------------------------ directional stage: specification
def dir_front(h, d, c=Consts.EXACT):
    """ref_model.py:80-82, 86-88 in h's dtype -> kinv (M, 1), normal (M, 3), n.d (M, 1), w_r (M, 3)"""
    kinv = F.softplus(h[:, 9:10] - 1.0)
    n0 = h[:, 0:3]
    n = -n0 / (n0.norm(dim=-1, keepdim=True) + c.eps_n)
    dot = torch.sum(d * n, dim=-1, keepdim=True)
    return kinv, n, dot, d - 2.0 * dot * n


def dir_forward(h, d, deg, c=Consts.EXACT):
    """the stage in h's dtype -> ([IDE real T | IDE imag T | n.d] (M, 2T + 1), normal (M, 3))"""
    kinv, n, dot, r = dir_front(h, d, c)
    return torch.cat((ide(r, kinv, deg), dot), dim=-1), n


def ide_magnitudes(r, kinv, deg):
    """fp64 -> A = att |w|^m |P|_t, dAz = att |w|^m sum k |mat| |z|^(k-1), dAw = att m |w|^(m-1) |P|_t, B = |w|^m |P|_t; each (M, T)"""
    terms, mat = ide_terms(deg)
    aw, az = torch.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2), r[:, 2].abs()
    A, dAz, dAw, B = [], [], [], []
    for t, (l, m) in enumerate(terms):
        att = torch.exp(-0.5 * l * (l + 1) * kinv[:, 0])
        P = sum(abs(float(mat[k, t])) * az ** k for k in range(l - m + 1))
        dP = sum(k * abs(float(mat[k, t])) * az ** (k - 1) for k in range(1, l - m + 1)) if l - m >= 1 else torch.zeros_like(az)
        A.append(att * aw ** m * P); dAz.append(att * aw ** m * dP); B.append(aw ** m * P)
        dAw.append(att * m * aw ** (m - 1) * P if m else torch.zeros_like(az))
    return tuple(torch.stack(v, dim=1) for v in (A, dAz, dAw, B))


def dir_forward_check(heads, dirs, deg, out_got, normal_got, c=Consts.KERNEL):
    """the three steps of the module docstring -> {"normal": report, "ndot": report, "ide": report}"""
    h, d = heads.detach().double().cpu(), dirs.detach().double().cpu()
    og, ng = out_got.detach().double().cpu(), normal_got.detach().double().cpu()
    T = T_of(deg)
    kinv, n, _, _ = dir_front(h, d, c)
    rep = {"normal": compare(ng, n, NORMAL_U * U * n.abs() + TINY)}
    dot_own = torch.sum(d * ng, dim=-1, keepdim=True)
    rep["ndot"] = compare(og[:, 2 * T:], dot_own, 3 * U * torch.sum((d * ng).abs(), dim=-1, keepdim=True) + TINY)
    dg = og[:, 2 * T:]
    r_own = d - 2.0 * dg * ng
    dr = 2.01 * U * (d.abs() + 2.0 * (dg * ng).abs())
    ide_ref = ide(r_own, kinv, deg)
    terms, _ = ide_terms(deg)
    A, dAz, dAw, B = ide_magnitudes(r_own, kinv, deg)
    l_ = torch.tensor([l for l, m in terms], dtype=torch.float64)
    m_ = torch.tensor([m for l, m in terms], dtype=torch.float64)
    sig = 0.5 * l_ * (l_ + 1)
    v = h[:, 9:10] - 1.0
    depth = 4 * m_ + 2 * l_ + 2 + att_depth(sig, kinv, v)
    tol = U * A * depth + 1.01 * (dAz * dr[:, 2:3] + dAw * (dr[:, 0:1] + dr[:, 1:2])) + TINY * (1 + B)
    rep["ide"] = compare(og[:, :2 * T], ide_ref, torch.cat((tol, tol), dim=1))
    return rep


# ------------------------------------------------------------------------------------------------ directional stage: explicit formulas
def ide_explicit(r, kinv, deg, mat, mut=()):
    """the kernel's evaluation order in r's dtype (powers by repeated multiplication, the polynomial term by term) -> (M, 2T).
    mut: "imag_sign" flips the sign of the imaginary part of term 1 (l = m = 1); "att" attenuates level 2 with l l / 2."""
    terms, _ = ide_terms(deg)
    lmax = 1 << (deg - 1)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    zp, re, im = [torch.ones_like(z)], [torch.ones_like(z)], [torch.zeros_like(z)]
    for k in range(1, lmax + 1):
        zp.append(zp[-1] * z)
        re_k = re[-1] * x - im[-1] * y
        im.append(re[-1] * y + im[-1] * x); re.append(re_k)
    outr, outi = [], []
    for t, (l, m) in enumerate(terms):
        s = 0.5 * (l * l if ("att" in mut and l == min(2, lmax)) else l * (l + 1))
        att = torch.exp(-s * kinv[:, 0])
        poly = torch.zeros_like(z)
        for k in range(l - m + 1):
            poly = poly + mat[k, t] * zp[k]
        outr.append((re[m] * poly) * att)
        outi.append((im[m] * poly) * att * (-1.0 if ("imag_sign" in mut and t == 1) else 1.0))
    return torch.cat((torch.stack(outr, 1), torch.stack(outi, 1)), dim=1)


def ide(r, kinv, deg):
    """oracle.ide_encode restated with integer powers by multiplication (equal to it to 1e-12 wherever it is finite, test_generic_ref_host.py).
    The oracle, like ref_func.py, raises x + i y to a TENSOR exponent: at x = y = 0 (w_r along +-z, one of the hand-made rows) torch
    returns NaN for (0 + 0 i)^0 and for every derivative there, where the function is the polynomial this evaluates."""
    return ide_explicit(r, kinv, deg, ide_terms(deg)[1].to(r.dtype))


def dir_forward_explicit(h, d, deg, c=Consts.KERNEL, mut=()):
    """torch evaluation in h's dtype of the stage as the kernel orders it -> (out (M, 2T + 1), normal).  mut: see ide_explicit;
    "refl2" drops the factor 2 of the reflection."""
    _, mat = ide_terms(deg)
    mat = mat.to(h.dtype)
    kinv = F.softplus(h[:, 9:10] - 1.0)
    n0 = h[:, 0:3]
    ln = torch.sqrt((n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1]) + n0[:, 2] * n0[:, 2])[:, None]
    n = -n0 / (ln + torch.tensor(c.eps_n, dtype=h.dtype))
    dot = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2])[:, None]
    r = d - (1.0 if "refl2" in mut else 2.0) * dot * n
    return torch.cat((ide_explicit(r, kinv, deg, mat, mut), dot), dim=1), n


def att_depth(sig, kinv, v):
    """relative error of att = expf(-sig kinv) in units of u: expf, the exponent's rounding, kinv's own error (softplus, v = rho - 1)"""
    return FN_U + sig * kinv * (1 + SP_U) + sig * v.abs() * torch.sigmoid(v)


def dir_backward_explicit(h, d, deg, d_out, g_n, c=Consts.KERNEL, mag=False, mut=(), att_err=False):
    """The adjoint as ref_dir_inputs_backward_kernel writes it, in h's dtype -> (M, 4) = d heads [0, 1, 2, 9].  mag=True: the magnitude
    pass (absolute values, sums for differences, |x + i y|^k for both parts of (x + i y)^k), evaluated at the true forward values.
    mut: "kinv_sig" leaves the factor sig out of d_kinv at level 2."""
    terms, mat = ide_terms(deg)
    mat = mat.to(h.dtype)
    T, lmax = len(terms), 1 << (deg - 1)
    ab = (lambda t: t.abs()) if mag else (lambda t: t)
    sub = (lambda a, b: a + b) if mag else (lambda a, b: a - b)
    v = h[:, 9] - 1.0
    kinv = F.softplus(v)
    n0 = h[:, 0:3]
    ln = torch.sqrt((n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1]) + n0[:, 2] * n0[:, 2])
    nn = ln + torch.tensor(c.eps_n, dtype=h.dtype)
    n = -n0 / nn[:, None]
    dot = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    r = d - 2.0 * dot[:, None] * n
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    if mag:
        mat, n, n0, d, d_out, g_n = mat.abs(), n.abs(), n0.abs(), d.abs(), d_out.abs(), g_n.abs()
        dot = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        aw, z = torch.sqrt(x * x + y * y), z.abs()
        re = [aw ** k for k in range(lmax + 1)]
        im, zp = re, [z ** k for k in range(lmax + 1)]
    else:
        zp, re, im = [torch.ones_like(z)], [torch.ones_like(z)], [torch.zeros_like(z)]
        for k in range(1, lmax + 1):
            zp.append(zp[-1] * z)
            re_k = re[-1] * x - im[-1] * y
            im.append(re[-1] * y + im[-1] * x); re.append(re_k)
    zero = torch.zeros_like(z)
    d_re, d_im = [zero] * (lmax + 1), [zero] * (lmax + 1)
    d_rz, d_kinv = zero, zero
    for t, (l, m) in enumerate(terms):
        sig = 0.5 * l * (l + 1)
        att = torch.exp(-sig * kinv)
        if att_err:
            att = att * att_depth(sig, kinv, v)
        poly, dpoly = zero, zero
        for k in range(l - m + 1):
            poly = poly + mat[k, t] * zp[k]
            if k >= 1:
                dpoly = dpoly + (k * mat[k, t]) * zp[k - 1]
        gr, gi = d_out[:, t], d_out[:, T + t]
        Aa = gr * re[m] + gi * im[m]
        d_rz = d_rz + Aa * att * dpoly
        d_kinv = sub(d_kinv, Aa * poly * (1.0 if ("kinv_sig" in mut and l == min(2, lmax)) else sig) * att)
        d_re[m] = d_re[m] + gr * poly * att
        d_im[m] = d_im[m] + gi * poly * att
    d_rx, d_ry = zero, zero
    for k in range(1, lmax + 1):
        d_rx = d_rx + k * (d_re[k] * re[k - 1] + d_im[k] * im[k - 1])
        d_ry = d_ry + k * sub(d_im[k] * re[k - 1], d_re[k] * im[k - 1])
    g_nd = d_out[:, 2 * T]
    dr = (d_rx, d_ry, d_rz)
    rdotn = (d_rx * n[:, 0] + d_ry * n[:, 1]) + d_rz * n[:, 2]
    dn = [sub(g_n[:, i] + g_nd * d[:, i], 2.0 * (rdotn * d[:, i] + ab(dot) * dr[i])) for i in range(3)]
    n0dn = (n0[:, 0] * dn[0] + n0[:, 1] * dn[1]) + n0[:, 2] * dn[2]
    cden = n0dn / (ln.clamp_min(1e-30) * nn * nn)
    cols = [(sub(dn[i] / nn, n0[:, i] * cden)) * (1.0 if mag else -1.0) for i in range(3)]
    cols.append(d_kinv * torch.sigmoid(v))
    return torch.stack(cols, dim=1)


def dir_backward_spec(heads, dirs, deg, d_out, g_normal, c=Consts.KERNEL):
    """-> (fp64 autograd adjoint (M, 4) w.r.t. head columns [0, 1, 2, 9], tol (M, 4))"""
    h = heads.detach().double().cpu().clone().requires_grad_(True)
    d, do, gn = dirs.detach().double().cpu(), d_out.detach().double().cpu(), g_normal.detach().double().cpu()
    out, n = dir_forward(h, d, deg, c)
    g, = torch.autograd.grad((out * do).sum() + (n * gn).sum(), h)
    A, A_att = dir_backward_magnitudes(h.detach(), d, deg, do, gn, c)
    nn = h.detach()[:, 0:3].norm(dim=-1, keepdim=True) + c.eps_n
    return g[:, [0, 1, 2, 9]], U * (DIR_BWD_C[deg] * A + A_att) + TINY * 1e4 / nn


def dir_backward_magnitudes(h, d, deg, d_out, g_n, c=Consts.KERNEL):
    """fp64 -> (A, A_att) (M, 4): the magnitude pass, and the same with every att_l multiplied by att_depth"""
    return (dir_backward_explicit(h, d, deg, d_out, g_n, c, mag=True), dir_backward_explicit(h, d, deg, d_out, g_n, c, mag=True, att_err=True))


def dir_backward_measure(got, heads, dirs, deg, d_out, g_normal, c=Consts.KERNEL):
    """the smallest C for which `got` is inside the bound: max over the elements of (err / u - A_att) / A"""
    ref, _ = dir_backward_spec(heads, dirs, deg, d_out, g_normal, c)
    A, A_att = dir_backward_magnitudes(heads.double(), dirs.double(), deg, d_out.double(), g_normal.double(), c)
    err = (got.detach().double().cpu() - ref).abs()
    return float((((err / U) - A_att) / A.clamp_min(1e-300)).clamp_min(0.0).max())


# ------------------------------------------------------------------------------------------------ colour combination
def srgb(lin, c):
    eps = torch.full((1,), torch.finfo(torch.float32).eps, dtype=lin.dtype)
    return torch.where(lin <= c.knee, c.c1292 * lin, (211 * torch.maximum(eps, lin) ** c.p512 - 11) / 200)


def combine_forward(h, pre, use_srgb, c=Consts.EXACT):
    """ref_model.py:98-105 in h's dtype from the spec head's PRE-activation -> rgbo (M, 4)"""
    spec = torch.sigmoid(pre) * torch.sigmoid(h[:, 6:9])
    rgb = srgb(spec + torch.sigmoid(h[:, 3:6] - c.log3), c) if use_srgb else spec + torch.sigmoid(h[:, 3:6])
    return torch.cat((rgb, h[:, 10:11]), dim=-1)


def _combine_parts(h, s, use_srgb, c):
    st = torch.sigmoid(h[:, 6:9])
    arg = h[:, 3:6] - c.log3 if use_srgb else h[:, 3:6]
    sd = torch.sigmoid(arg)
    lin = s * st + sd
    shift = U * arg.abs() * sd * (1 - sd) if use_srgb else torch.zeros_like(sd)
    tol_lin = U * ((SIG_U + 2) * s * st + (SIG_U + 1) * sd) + shift
    return st, sd, lin, tol_lin, SIG_U * U + (U * arg.abs() * (1 - sd) if use_srgb else 0.0)


def combine_spec(heads, spec, use_srgb, c=Consts.KERNEL):
    """-> (fp64 rgbo (M, 4), tol (M, 4)) from the kernel's inputs: heads and spec = sigmoid(spec head) as the product wrote it"""
    h, s = heads.detach().double().cpu(), spec.detach().double().cpu()
    st, sd, lin, tol_lin, _ = _combine_parts(h, s, use_srgb, c)
    if not use_srgb:
        ref, tol = lin, tol_lin
    else:
        assert bool(((lin - c.knee).abs() > 10 * tol_lin).all()), "an input row sits on the knee: the side would be ambiguous"
        ref = srgb(lin, c)
        pw = 211 * lin.clamp_min(2.0 ** -23) ** c.p512
        above = (pw * ((FN_U + 1) * U + c.p512 * tol_lin / lin.clamp_min(2.0 ** -23)) + U * (pw - 11).abs()) / 200 + 2 * U * ref.abs()
        tol = torch.where(lin <= c.knee, c.c1292 * tol_lin + U * ref.abs(), above)
    return torch.cat((ref, h[:, 10:11]), dim=1), torch.cat((tol, torch.zeros_like(h[:, 10:11])), dim=1)


def combine_backward_spec(g_rgbo, heads, spec, use_srgb, c=Consts.KERNEL):
    """-> (d_spec (M, 3) w.r.t. the spec head's pre-activation, tol), (d_heads columns [3..8, 10] (M, 7), tol): fp64 autograd of
    combine_forward at pre = logit(spec)"""
    h, s, g = heads.detach().double().cpu(), spec.detach().double().cpu(), g_rgbo.detach().double().cpu()
    st, sd, lin, tol_lin, eps_sd = _combine_parts(h, s, use_srgb, c)
    # autograd through sigmoid(pre) needs a pre with sigmoid(pre) == s; s in {0, 1} has none, and its adjoint s (1 - s) is exactly 0:
    # differentiate w.r.t. s and apply the factor s (1 - s) explicitly
    hh, ss = h.clone().requires_grad_(True), s.clone().requires_grad_(True)
    spec_t = ss * torch.sigmoid(hh[:, 6:9])
    rgb = srgb(spec_t + torch.sigmoid(hh[:, 3:6] - c.log3), c) if use_srgb else spec_t + torch.sigmoid(hh[:, 3:6])
    out = torch.cat((rgb, hh[:, 10:11]), dim=-1)
    gh, gs = torch.autograd.grad((out * g).sum(), (hh, ss))
    d_spec = gs * (s * (1 - s))
    if use_srgb:
        slope = torch.where(lin <= c.knee, torch.full_like(lin, c.c1292), (211 / 200) * c.p512 * lin.clamp_min(2.0 ** -23) ** (-c.p712))
        drift = abs(c.p512 - 1 + c.p712) * lin.clamp_min(2.0 ** -23).log().abs()      # the kernel's slope exponent is fl32(7/12), not 1 - fl32(5/12)
        eps_gl = torch.where(lin <= c.knee, torch.full_like(lin, U), (1 + FN_U + 3) * U + c.p712 * tol_lin / lin.clamp_min(2.0 ** -23) + drift)
    else:
        slope, eps_gl = torch.ones_like(lin), torch.full_like(lin, U)
    gl = (g[:, :3] * slope).abs()
    e_q = lambda y, e: y * (e * (1 - 2 * y).abs() + 2 * U * (1 - y))
    t_spec = d_spec.abs() * (eps_gl + (SIG_U + 4) * U) + TINY
    t_dif = gl * e_q(sd, eps_sd) + gh[:, 3:6].abs() * (eps_gl + U) + TINY
    t_tint = gl * s * e_q(st, SIG_U * U) + gh[:, 6:9].abs() * (eps_gl + 2 * U) + TINY
    return (d_spec, t_spec), (torch.cat((gh[:, 3:9], gh[:, 10:11]), dim=1), torch.cat((t_dif, t_tint, torch.zeros_like(gh[:, 10:11])), dim=1))


def combine_explicit(h, s, use_srgb, c=Consts.KERNEL, g=None, mut=()):
    """torch evaluation in h's dtype as the kernels order it: forward (g None) -> rgbo; backward -> (d_spec, d_heads [3..8, 10]).
    mut: "slope_side" takes srgb_slope on the wrong side of the knee for row 0."""
    k = lambda v: torch.tensor(v, dtype=h.dtype)
    st = torch.sigmoid(h[:, 6:9])
    sd = torch.sigmoid(h[:, 3:6] - k(c.log3)) if use_srgb else torch.sigmoid(h[:, 3:6])
    lin = s * st + sd
    eps = torch.full((1,), torch.finfo(torch.float32).eps, dtype=h.dtype)
    if g is None:
        rgb = torch.where(lin <= k(c.knee), k(c.c1292) * lin, (211 * torch.maximum(eps, lin) ** k(c.p512) - 11) / 200) if use_srgb else lin
        return torch.cat((rgb, h[:, 10:11]), dim=1)
    if use_srgb:
        below = lin <= k(c.knee)
        if "slope_side" in mut:
            below = below.clone(); below[0] = ~below[0]
        slope = torch.where(below, k(c.c1292).expand_as(lin), k(211 / 200 * c.p512) * torch.maximum(eps, lin) ** (-k(c.p712)))
        gl = g[:, :3] * slope
    else:
        gl = g[:, :3]
    return (gl * st) * (s * (1 - s)), torch.cat((gl * (sd * (1 - sd)), (gl * s) * (st * (1 - st)), g[:, 3:4]), dim=1)


# ------------------------------------------------------------------------------------------------ positional encoding
def pe_forward(x, L, cat_origin):
    """[x | sin 2^0 x | cos 2^0 x | sin 2^1 x | ...] rows in x's dtype"""
    parts = [x] if cat_origin else []
    for f in range(L):
        a = (2.0 ** f) * x
        parts += [torch.sin(a), torch.cos(a)]
    return torch.cat(parts, dim=-1)


def pe_backward_spec(d_enc, x, L, cat_origin):
    """-> (fp64 autograd adjoint (M, 3), tol): the sine arguments 2^f x32 are formed exactly (a power of two times an fp32 number)"""
    de = d_enc.detach().double().cpu()
    xx = x.detach().double().cpu().clone().requires_grad_(True)
    g, = torch.autograd.grad((pe_forward(xx, L, cat_origin) * de).sum(), xx)
    xd, off = xx.detach(), 3 if cat_origin else 0
    A = de[:, :3].abs() if cat_origin else torch.zeros_like(xd)
    for f in range(L):
        a = (2.0 ** f) * xd
        A = A + (2.0 ** f) * ((torch.cos(a) * de[:, off + 6 * f: off + 6 * f + 3]).abs() + (torch.sin(a) * de[:, off + 6 * f + 3: off + 6 * f + 6]).abs())
    return g, (L + 7) * U * A + TINY


def pe_backward_explicit(d_enc, x, L, cat_origin, mut=()):
    """the kernel's sum in x's dtype.  mut: "octave" leaves the factor 2^f out at f = 2."""
    off = 3 if cat_origin else 0
    acc = d_enc[:, :3].clone() if cat_origin else torch.zeros_like(x)
    for f in range(L):
        a = (2.0 ** f) * x
        sc = 1.0 if ("octave" in mut and f == 2) else 2.0 ** f
        acc = acc + sc * (torch.cos(a) * d_enc[:, off + 6 * f: off + 6 * f + 3] - torch.sin(a) * d_enc[:, off + 6 * f + 3: off + 6 * f + 6])
    return acc


# ------------------------------------------------------------------------------------------------ scene contraction
def contract_spec(x, grad=None):
    """-> (fp64 oracle.contract(x32) or its autograd pull-back of grad, tol) (M, 3)"""
    xx = x.detach().double().cpu().clone().requires_grad_(True)
    out = O.contract(xx)
    r = xx.detach().norm(dim=-1, keepdim=True)
    if grad is None:
        return out.detach(), CONTRACT_FWD_U * U * out.detach().abs() + TINY
    g = grad.detach().double().cpu()
    pb, = torch.autograd.grad((out * g).sum(), xx)
    rr = r.clamp_min(1.0)
    k = (2.0 - 1.0 / rr) / rr
    u = xx.detach().abs() / r.clamp_min(1e-300)
    A = torch.where(r > 1.0, k * g.abs() + (u * g.abs()).sum(-1, keepdim=True) * (1.0 / (rr * rr) + k) * u, g.abs())
    return pb, CONTRACT_BWD_U * U * A + TINY


# ------------------------------------------------------------------------------------------------ layer product
def gemm_spec(a, b, prec, bias=None, act=0, mask=None, pre=None):
    """C = act(a b + bias) * [mask > 0] in fp64 from fp32 views a (M, P), b (P, N) (rounded to bf16 first when prec == "bf16") and the
    per-element bound (P + 2) u sum |a b| (+ |bias|) carried through the activation.  pre = (a b, |a| |b|) already formed in fp64 from the
    rounded operands (a long contraction shared by several calls).  -> (ref, tol)"""
    q = (lambda t: t.detach().cpu().bfloat16().double()) if prec == "bf16" else (lambda t: t.detach().cpu().double())
    P = a.shape[1]
    if pre is None:
        A, B = q(a), q(b)
        pre = (A @ B, A.abs() @ B.abs())
    s, mag = pre
    if bias is not None:
        bb = bias.detach().cpu().double().reshape(1, -1)
        s, mag = s + bb, mag + bb.abs()
    tol = (P + 2) * U * mag + (P + 1) * TINY
    if act == 1:
        s = s.clamp_min(0.0)
    elif act == 2:
        y = torch.sigmoid(s)
        s, tol = y, 1.01 * y * (1 - y) * tol + SIG_U * U * y + TINY
    if mask is not None:
        on = mask.detach().cpu() > 0                                     # the kernel's rule: !(mask > 0) -> 0 (NaN, -0.0, +0.0 close it)
        s, tol = torch.where(on, s, torch.zeros_like(s)), torch.where(on, tol, torch.zeros_like(tol))
    return s, tol


# ------------------------------------------------------------------------------------------------ the whole RefNeRF, composed of the stages
def ref_forward_composed(sd, pts, Lp, deg, use_srgb, cat_origin):
    """RefNeRF.forward from the per-stage specifications above with plain matmuls for the layer products, in pts' dtype;
    pts (M, 6) -> (rgbo (M, 4), normal (M, 3)).  Must equal oracle.ref_forward (tests/test_generic_ref_host.py)."""
    lin = lambda name, t: t @ sd[name + ".weight"].t() + sd[name + ".bias"]
    x, d = pts[:, :3], pts[:, 3:]
    ex = pe_forward(x, Lp, cat_origin)
    h = ex
    for i in (0, 2, 4, 6):
        h = F.relu(lin("spa_block1.%d" % i, h))
    g = torch.cat((ex, h), dim=-1)
    for i in (0, 2, 4, 6):
        g = F.relu(lin("spa_block2.%d" % i, g))
    heads = torch.cat((lin("norm_col_tint_head", g), lin("rho_tau_head", g)), dim=-1)            # the kernels' 11 head columns
    dir_in, normal = dir_forward(heads, d, deg)
    allin = torch.cat((lin("bottle_neck", g), dir_in), dim=-1)
    r = allin
    for i in (0, 2, 4, 6):
        r = F.relu(lin("dir_block1.%d" % i, r))
    r = torch.cat((allin, r), dim=-1)
    for i in (0, 2, 4, 6):
        r = F.relu(lin("dir_block2.%d" % i, r))
    return combine_forward(heads, lin("spec_rgb_head.0", r), use_srgb), normal
