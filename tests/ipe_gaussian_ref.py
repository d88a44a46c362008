"""The fp64 specification of the integrated positional encoding under the Mip-NeRF 360 scene contraction of the WHOLE frustum Gaussian
(nerf_amd_samples.contract = NERF_AMD_CONTRACT_GAUSSIAN, nerf_amd_ipe_feature_gaussian), and the derivation of every per-element bound
the GPU tests hold the fp32 / bf16 kernels to.  Plain helper module (no fixtures), in the manner of forward_ref.py; nothing here is taken
from the package: tests/test_ipe_gaussian_host.py checks the closed form against autograd and shows that the comparator reports four
planted faults, tests/test_gpu_ipe_gaussian.py feeds it what the kernels wrote.

THE DEFINITION (`spec`).  The reference's Gaussian of a conical frustum (mip_methods.py:15-33, with its quirk that dn is the norm of the
whole (N,3) direction tensor):

    mid = (z0 + z1) / 2, hw = (z1 - z0) / 2, t1 = 3 mid^2 + hw^2
    mu_t  = mid + 2 mid hw^2 / t1
    var_t = hw^2 / 3 - 4 hw^4 (12 mid^2 - hw^2) / (15 t1^2)
    var_r = r^2 (mid^2 / 4 + 5 hw^2 / 12 - 4 hw^4 / (15 t1))
    x = o + mu_t d,   Sigma = (var_t - var_r / dn) d d^T + var_r I,   diag Sigma = var_t d^2 + var_r (1 - d^2 / dn)

pushed through the linearised contraction f(x) = x for |x| <= 1, (2 - 1/|x|) x / |x| otherwise (Barron et al. 2022, eq. 10-14).  With
n = |x| > 1:   k = (2 n - 1) / n^2,  a = 2 (1 - n) / n^4,  J = k I + a x x^T (symmetric),

    Jd = k d + a x (x.d),    (J J^T)_cc = k^2 + (2 k a + a^2 n^2) x_c^2
    var'_c = (J Sigma J^T)_cc = var_t (Jd)_c^2 + var_r ((J J^T)_cc - (Jd)_c^2 / dn),      mu' = f(x)

and for n <= 1: mu' = x, var' = diag Sigma.  feat[6 l + 3 t + c] = (t ? cos : sin)(2^l mu'_c) exp(-0.5 4^l var'_c).  mode "metric" is the
earlier definition (contract = 1): mu' = f(x), var' = diag Sigma everywhere.

WHAT HOLDS BETWEEN THE TWO MODES.  J is symmetric with eigenvalues k (twice) and 1 / n^2, all <= 1, so tr(J Sigma J^T) = tr(J^2 Sigma)
<= tr(Sigma): the SUM of the three variances never grows, and per level the PRODUCT over the coordinates of the attenuations never
shrinks.  A single coordinate can grow: (J Sigma J^T)_cc = v^T Sigma v with v = J e_c, which is shorter than e_c but turned towards the
ray, and Sigma is strongly anisotropic (var_t >> var_r); with origins in [-0.5, 0.5]^3 about one element in a hundred does, by up to an
order of magnitude.  Only for a ray through the origin (x parallel to d: J and Sigma commute) is var'_c <= var_c true for every c -- the
case the element-wise statement was first checked on.  The tests therefore assert the element-wise inequality on rays through the
origin (`radial`) and the trace / product form on every ray (`att2`).

THE BOUNDS (`kernel_bounds`).  The kernels compute the same quantities in fp32, so the bound on an output is the forward error of an
fp32 evaluation -- a property of the number format and of the sequence of operations, not of what any kernel returned.  It is obtained
mechanically: `Fl` carries, next to the exact value v of a quantity (fp64), a bound e on |computed - v|, and every operation propagates
the operands' bounds to first order WITH the second-order terms kept (so the result is a true upper bound, not an estimate) and adds its
own rounding:

    a + b:   e = e_a + e_b                             + u (|v| + e) + 2^-126
    a * b:   e = |a| e_b + |b| e_a + e_a e_b           + u (|v| + e) + 2^-126          (fma(a, b, c): + e_c, ONE rounding)
    a / b:   e = (e_a + |a / b| e_b) / (|b| - e_b)     + 5 u (|v| + e) + 2^-126        (2.5 ulp: the bound forward_ref.py uses)
    sqrt a:  e = e_a / (sqrt(max(a - e_a, 0)) + sqrt a) + 4 u (|v| + e)                (2 ulp)
    2^j a:   exact
    sin, cos a:  e = e_a + max(4 u, D(|a|))     1-Lipschitz, plus the error of device_common.h sin_quadrant at an argument of that size.
                                   D is derived operation by operation below (SIN_QUADRANT); D <= 4 u for |a| <= 2^21, so the constant
                                   4 u this module has always used stands there (here |a| <= 2^9 . 2) and D takes over beyond
    exp a (a <= 0):  e = e_a exp(v + e_a) + 6 u exp(v + e_a)       mean value theorem with the LARGER of the two exponentials; 3 ulp
                                   (forward_ref.py's figure for expf)

u = 2^-24; 2^-126 pays for a result flushed or denormalised.  The sequence of operations is the one device_common.h states in prose
(cone_moments, cone_mean_cov, and for the contracted Gaussian the tangential / radial split

    t = 1 / n, k = (2 - t) / n, xh = x t, Jd = k (d - xh (xh.d)) + xh ((xh.d) t^2),
    (J J^T)_cc = k^2 (xh_a^2 + xh_b^2) + xh_c^2 t^4            (a, b the other two coordinates)

which the issue asks for because k d and a x (x.d) nearly cancel along the ray); it is restated here operation by operation, so the
cancellation that remains in d - xh (xh.d) -- an absolute error of about u |d| against a result of size |d| |o_perp| / n -- is IN the bound:
it grows with n exactly as the rounding does.  That error is harmless where it is large: it enters var' multiplied by var_t k^2 ~ 1 / n^2.
The exact values v are formed by the same sequence in fp64 and agree with `spec` to fp64 rounding (asserted on the host).

From mu' +- E_mu and var' +- E_var to a feature, the issue's first-order terms fall out of the same propagation: the argument 2^l mu'
carries 2^l E_mu, the exponent 0.5 4^l var' carries 0.5 4^l E_var and the exponential turns it into 0.5 4^l E_var att, sin / cos / exp add
their evaluation errors, the product rounds once.
  path "direct" (the fp32 kernels and the stand-alone encoder): every level from its own range reduction and its own expf.
  path "doubling" (the bf16 fused kernels, mlp_kernels.hip encode_ipe): level 0 as above, then per level s' = (2 s) c, c' = fma(-2 s, s, 1),
      att' = (att^2)^2.  The exact values obey the same identities, so v stays the specification's and e grows by about 2x (angle) and
      4x (attenuation, relative) per level -- which is what the recurrences do to an error.
  `stored_bf16`: the dump element is the fp32 value rounded to nearest bf16: + 2^-8 (|v| + e)  (forward_ref.py's operand rounding).
The branch n > 1 is taken on the fp32 norm: a frustum whose metric mean lies within 1e-4 of the unit sphere could take the other branch
than fp64 does, so the GPU tests assert that their inputs have none (`sphere_gap`).

THE COMPARATOR (`compare`): max(err / tol) over every element of feat and mu', and -- because inside the unit ball the Gaussian mode must
return the bits of contract = 1, which no tolerance can see -- the number of elements of inside-ball frusta whose bits differ from the
metric twin's.  None of these is fitted to what the kernels produce.

SIN_QUADRANT (`sincos_abs`): the error of sin_quadrant / sincos_quadrant (device_common.h) as a function of the argument's size.  With
q = |a| 2 / pi (a real number), u = 2^-24:
  k = rint(fl(a c0)), c0 = fl(2 / pi) = (2 / pi) (1 + e0), e0 = -4.0342e-8; the product rounds once, so |fl(a c0) - a 2 / pi| <= ETA q with
      ETA = |e0| + u + |e0| u < 1.0e-7, and rint moves it by at most 1/2:   |a 2 / pi - k| <= 1/2 + ETA q.
      Near a half-integer of a 2 / pi, k can therefore be the OTHER neighbour: the reduced argument r = a - k pi / 2 is then no longer
      inside [-pi/4, pi/4] but inside |r| <= R(q) = (pi / 2) (1/2 + ETA q): 0.7887 at |a| = 2^15, 0.995 at |a| = 2^21.
  r1 = fma(-k, C1, a), C1 = fl(pi / 2) = m 2^-23:  EXACT.  For |a| >= 1, a and k C1 are multiples of 2^-23 and |a - k C1| <= R + |k| |pi/2 - C1|
      (4.38e-8 |k|) < 2, so the difference has at most 24 bits; for |a| < 1, k is 0 (r1 = a) or +-1 (|a| >= 0.78: a multiple of 2^-24 minus a
      multiple of 2^-23, below 1 in size).  This holds while R(q) + 4.38e-8 |k| < 2, i.e. for |k| < 6.0e6 -- far beyond the domain below.
  r2 = fma(-k, C2, r1), r3 = fma(-k, C3, r2):  each rounds once, |delta| <= u |exact| <= u R (1 + 2^-20)   (|k C3| <= 2^21 . 1.8e-15).
  C1 + C2 + C3 = pi / 2 - rho, |rho| = 1.06e-23 < 2^-72 (exact rational arithmetic on the three literals, re-done in
      tests/test_encoding_ref_host.py): r3 = (a - k pi / 2) + k rho + delta2 + delta3, |k| <= q (1 + ETA) + 1/2.
  z = fl(r r);  sine: five fma for ps (|ps| <= 1/6, its error <= 2 u / 6 with room), w = fl(r z) (2 u relative), s = fma(w, ps, r):
      |s - P_s(r)| <= 2 u |r|^3 / 6 + |r|^3 2 u / 6 + u |s| <= u (|sin r| + 0.67 |r|^3);
      cosine: zz = fl(z z) (3 u relative), five fma for pc (|pc| <= 1/24, error <= 2 u / 24), h = fma(-1/2, z, 1) (u r^2 / 2 + u |h|, and
      |h| = 1 - r^2 / 2 for |r| <= 1.2), c = fma(zz, pc, h):   |c - P_c(r)| <= u (1 + |cos r| + 0.21 r^4).
  P_s, P_c: the two polynomials with their fp32 coefficients against sin and cos on |r| <= 1.2, evaluated in fp64 on two million points
      (a property of the coefficients, not of a kernel): 0.126 u and 0.042 u; allowed POLY_APPROX = 0.25 u.
  The quadrant selects +-s or +-c exactly.  Both |r|-dependent sums grow with |r|, so with R' = R(q) (1 + 2^-20):
      D(|a|) = u (2 R' + max(1 + cos R' + 0.21 R'^4, sin R' + 0.67 R'^3) + 0.25) + (q (1 + ETA) + 1/2) 2^-72
  = 3.61 u at |a| = 2^15 (the range device_common.h documents), 3.88 u at 1.54e6 = 2^9 . 1000 . 3 (disparity spacing to far = 1000, |d| = 3,
  no contraction) and 3.99 u at 2^21; just beyond, it passes 4 u.  SINCOS_DOMAIN = 2^21 is the range over which this derivation is used
  as a PROOF (R(2^21) = 0.995 lies inside the |r| <= 1.2 of the polynomial sup): `sincos_abs` refuses a larger argument.  No descriptor
  field bounds far or |d|, so the domain is a contract of the entry points: include/nerf_amd.h states it."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
BF16_HALF_ULP = 2.0 ** -8
DIV_U, SQRT_U, EXP_U, SINCOS_ABS = 5 * U, 4 * U, 6 * U, 4 * U
SINCOS_ETA = 4.0342060334366545e-08 * (1 + U) + U      # |fl(a c0) - a 2 / pi| <= SINCOS_ETA |a| 2 / pi
SINCOS_RHO = 2.0 ** -72                                # >= |pi / 2 - C1 - C2 - C3|
SINCOS_DOMAIN = 2.0 ** 21                              # the largest |a| for which sincos_abs is a proof
POLY_APPROX = 0.25 * U                                 # >= sup |P(r) - sin / cos r| on |r| <= POLY_RANGE (measured 0.126 u, 0.042 u)
POLY_RANGE = 1.2
FIVE_TWELFTHS_F32 = 0.4166666567325592          # the constant of the reference's fp32 arithmetic (the specification uses 5 / 12)


# ------------------------------------------------------------------------------------------------ the specification
def cone_moments(z):
    z = z.double()
    z0, z1 = z[:, :-1], z[:, 1:]
    mid, hw2 = (z1 + z0) / 2, ((z1 - z0) / 2) ** 2
    t1 = 3 * mid ** 2 + hw2
    mu_t = mid + 2 * mid * hw2 / t1
    var_t = hw2 / 3 - 4 * (hw2 ** 2) * (12 * mid ** 2 - hw2) / 15 / (t1 ** 2)
    var_r_unit = 0.25 * mid ** 2 + 5 / 12 * hw2 - 4 * hw2 ** 2 / (15 * t1)
    return mu_t, var_t, var_r_unit


def contract(x):
    n = x.norm(dim=-1, keepdim=True)
    return torch.where(n > 1, (2 - 1 / n.clamp_min(1e-300)) / n.clamp_min(1e-300), torch.ones_like(n)) * x


def gaussian(z, rays, r2, dn):
    """-> metric mean x (N,S,3), metric diag Sigma (N,S,3), var_t, var_r (N,S,1), d (N,1,3): fp64"""
    mu_t, var_t, vru = cone_moments(z)
    var_r = float(r2) * vru
    o, d = rays[:, None, :3].double(), rays[:, None, 3:6].double()
    x = o + mu_t[..., None] * d
    var_t, var_r = var_t[..., None], var_r[..., None]
    dd = d * d
    diag = var_t * dd + var_r * (1 - dd / float(dn))
    return x, diag, var_t, var_r, d


def pushed_variance(x, d, var_t, var_r, dn):
    """the closed form of the definition for n > 1 (evaluated wherever asked: the caller selects)"""
    n2 = (x * x).sum(-1, keepdim=True)
    n = n2.sqrt()
    k, a = (2 * n - 1) / n2, 2 * (1 - n) / (n2 * n2)
    jd = k * d + a * x * (x * d).sum(-1, keepdim=True)
    jj = k * k + (2 * k * a + a * a * n2) * x * x
    return var_t * jd * jd + var_r * (jj - jd * jd / float(dn))


def lift(mu, var, L):
    f2 = torch.tensor([2.0 ** l for l in range(L)], dtype=torch.float64)[:, None]
    arg = f2 * mu[..., None, :]                                                          # (N,S,L,3)
    att = torch.exp(-0.5 * (f2 * f2) * var[..., None, :])
    return torch.cat((torch.sin(arg) * att, torch.cos(arg) * att), dim=-1).reshape(mu.shape[0], mu.shape[1], 6 * L)


def spec(z, rays, L, r2, dn, mode="gaussian"):
    """z (N,S+1), rays (N,6) fp32 (CPU), r2 = the fp32 square of the pixel radius, dn = the fp32 direction norm the kernel read.
    -> feat (N,S,6L), mu' (N,S,3), var' (N,S,3) in fp64.  mode: "gaussian" (the definition above), "metric" (contract = 1) or "plain"
    (contract = 0: the reference's ipe_feature, neither mean nor covariance contracted)."""
    x, diag, var_t, var_r, d = gaussian(z, rays, r2, dn)
    var = diag
    if mode == "gaussian":
        outside = x.norm(dim=-1, keepdim=True) > 1
        safe = torch.where(outside, x, torch.full_like(x, 2.0))
        var = torch.where(outside, pushed_variance(safe, d, var_t, var_r, dn), diag)
    mu = x if mode == "plain" else contract(x)
    return lift(mu, var, L), mu, var


def sphere_gap(z, rays):
    """min | |x| - 1 | over the metric means"""
    mu_t = cone_moments(z)[0]
    x = rays[:, None, :3].double() + mu_t[..., None] * rays[:, None, 3:6].double()
    return float((x.norm(dim=-1) - 1).abs().min())


def radial(rays):
    """the same directions from the origin: x is parallel to d, J and Sigma commute"""
    out = rays.clone()
    out[:, :3] = 0
    return out


def att2(feat, L):
    """feat (N,S,6L) -> sin^2 + cos^2 = the squared attenuation per (level, coordinate): (N,S,L,3)"""
    f = feat.double().reshape(feat.shape[0], feat.shape[1], L, 2, 3)
    return (f * f).sum(3)


# ------------------------------------------------------------------------------------------------ the inputs
FAMILIES = ("inside", "straddle", "far")
SPHERE_GAP = 1e-4


def depths(rays, S, family, gen):
    """(N, S + 1) sorted depths.  inside: every point of the ray segment stays in the unit ball (|o| + z |d| < 1); straddle: z from about
    0.5 to 6; far: geometric from 0.2 out to 1e6 (what disparity spacing produces), each ray scaled by a factor in [0.9, 1.1]"""
    N = rays.shape[0]
    o, d = rays[:, :3].double().norm(dim=-1, keepdim=True), rays[:, 3:6].double().norm(dim=-1, keepdim=True)
    if family == "inside":
        z = (torch.sort(torch.rand(N, S + 1, generator=gen, dtype=torch.float64), dim=-1)[0] * 0.88 + 0.02) * (1 - o) / d
    elif family == "straddle":
        z = torch.sort(torch.rand(N, S + 1, generator=gen, dtype=torch.float64) * 5.5 + 0.5, dim=-1)[0]
    else:
        z = 0.2 * (1e6 / 0.2) ** (torch.arange(S + 1, dtype=torch.float64) / S)[None, :] * (0.9 + 0.2 * torch.rand(N, 1, generator=gen, dtype=torch.float64))
    return z.float().contiguous()


def make_inputs(N, S, seed=0, need_gap=True):
    """-> (rays (N,6): origins in [-0.5, 0.5]^3, unnormalised randn directions; {family: z (N, S+1)}; the seed used).  The seed is the
    first from `seed` on for which |d|^2 < dn holds for every ray (dn = the norm of the whole direction tensor; the Gaussian's
    covariance is positive definite only then) and, with need_gap, no metric mean of any family lies within SPHERE_GAP of the unit
    sphere -- so no ray has to be left out."""
    for s in range(seed, seed + 256):
        gen = torch.Generator().manual_seed(s)
        rays = torch.cat((torch.rand(N, 3, generator=gen) - 0.5, torch.randn(N, 3, generator=gen)), -1).contiguous()
        d2 = (rays[:, 3:].double() ** 2).sum(-1)
        if not bool((d2 < d2.sum().sqrt().float().double()).all()):
            continue
        zs = {f: depths(rays, S, f, gen) for f in FAMILIES}
        if need_gap and min(sphere_gap(z, rays) for z in zs.values()) < SPHERE_GAP:
            continue
        return rays, zs, s
    raise AssertionError("no seed in %d .. %d gives admissible rays" % (seed, seed + 255))


# ------------------------------------------------------------------------------------------------ the bounds
class Fl:
    """a quantity an fp32 program computed: v = its exact value (fp64 tensor), e >= |computed - v|"""

    def __init__(self, v, e=None):
        self.v = v if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else (e if isinstance(e, torch.Tensor) else torch.full_like(self.v, float(e)))

    def _rounded(self, v, e, ru):
        return Fl(v, e + ru * (v.abs() + e) + TINY)

    def __add__(self, o):
        o = _fl(o)
        return self._rounded(self.v + o.v, self.e + o.e, U)

    def __sub__(self, o):
        o = _fl(o)
        return self._rounded(self.v - o.v, self.e + o.e, U)

    def __mul__(self, o):
        o = _fl(o)
        return self._rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e, U)

    def __truediv__(self, o):
        o = _fl(o)
        q = self.v / o.v
        den = o.v.abs() - o.e
        assert bool((den > 0).all()), "a divisor's bound reaches zero"
        return self._rounded(q, (self.e + q.abs() * o.e) / den, DIV_U)

    def scaled(self, p):                                   # by a power of two: exact
        return Fl(self.v * p, self.e * abs(p))

    def sqrt(self):
        r = self.v.sqrt()
        return self._rounded(r, self.e / ((self.v - self.e).clamp_min(0).sqrt() + r).clamp_min(1e-300), SQRT_U)

    def where(self, cond, other):
        return Fl(torch.where(cond, self.v, other.v), torch.where(cond, self.e, other.e))

    def stored_bf16(self):
        return Fl(self.v, self.e + BF16_HALF_ULP * (self.v.abs() + self.e))


def _fl(x):
    return x if isinstance(x, Fl) else Fl(x)


def fma(a, b, c):
    a, b, c = _fl(a), _fl(b), _fl(c)
    return a._rounded(a.v * b.v + c.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + c.e, U)


def sincos_reduced_range(mag):
    """R(q) of SIN_QUADRANT: the bound on |a - k pi / 2| for an argument of size mag (a float64 tensor)"""
    return (math.pi / 2) * (0.5 + SINCOS_ETA * mag * (2 / math.pi))


def sincos_derived(mag):
    """D(|a|) of SIN_QUADRANT (module docstring) for an argument of size mag <= SINCOS_DOMAIN"""
    q = mag * (2 / math.pi)
    R = sincos_reduced_range(mag) * (1 + 2.0 ** -20)
    poly = torch.maximum(1 + torch.cos(R) + 0.21 * R ** 4, torch.sin(R) + 0.67 * R ** 3)
    return U * (2 * R + poly) + POLY_APPROX + (q * (1 + SINCOS_ETA) + 0.5) * SINCOS_RHO


def sincos_abs(a):
    """the bound on |sin_quadrant(computed a) - sin(computed a)|: the constant 4 u wherever the derivation stays below it"""
    mag = a.v.abs() + a.e
    assert bool((mag <= SINCOS_DOMAIN).all()), "an argument of sin_quadrant beyond 2^21: outside the range the bound is derived for"
    return sincos_derived(mag).clamp_min(SINCOS_ABS)


def fl_sin(a):
    return Fl(torch.sin(a.v), a.e + sincos_abs(a))


def fl_cos(a):
    return Fl(torch.cos(a.v), a.e + sincos_abs(a))


def fl_exp(a):
    hi = torch.exp(a.v + a.e)
    return Fl(torch.exp(a.v), a.e * hi + EXP_U * hi + TINY)


def fl_moments(z, r2):
    z = z.double()
    z0, z1 = Fl(z[:, :-1, None]), Fl(z[:, 1:, None])
    mid, hw = (z1 + z0).scaled(0.5), (z1 - z0).scaled(0.5)
    hw2, mid2 = hw * hw, mid * mid
    t1 = mid2 * 3.0 + hw2
    mu_t = mid + (mid.scaled(2.0) * hw2) / t1
    hw4 = hw2 * hw2
    var_t = hw2 / 3.0 - ((hw4.scaled(4.0) * (mid2 * 12.0 - hw2)) / 15.0) / (t1 * t1)
    c512 = Fl(torch.tensor(5.0 / 12.0, dtype=torch.float64), abs(5.0 / 12.0 - FIVE_TWELFTHS_F32))
    var_r = Fl(float(r2)) * ((mid2.scaled(0.25) + c512 * hw2) - hw4.scaled(4.0) / (t1 * 15.0))
    return mu_t, var_t, var_r


def fl_gaussian(z, rays, r2, dn, mode):
    """-> (mu', var') as Fl of shape (N,S,3): the operations of cone_moments, cone_mean_cov and the contracted Gaussian, in their order.
    mode "plain": cone_mean_cov's values as they are (contract = 0)"""
    mu_t, var_t, var_r = fl_moments(z, r2)
    o, d, dn = Fl(rays[:, None, :3].double()), Fl(rays[:, None, 3:6].double()), Fl(float(dn))
    x = o + mu_t * d
    dd = d * d
    diag = var_t * dd + var_r * (Fl(1.0) - dd / dn)
    if mode == "plain":                                                                  # no contraction at all
        return x, diag
    xs = [Fl(x.v[..., c: c + 1], x.e[..., c: c + 1]) for c in range(3)]
    ds = [Fl(d.v[..., c: c + 1]) for c in range(3)]
    n = ((xs[0] * xs[0] + xs[1] * xs[1]) + xs[2] * xs[2]).sqrt()
    outside = n.v > 1
    n = n.where(outside, Fl(torch.full_like(n.v, 2.0)))                               # (the branch not taken is computed on a harmless n)
    t = Fl(1.0) / n
    kk = (Fl(2.0) - t) / n
    mu = (x * kk).where(outside, x)
    if mode == "metric":
        return mu, diag
    xh = [xc * t for xc in xs]
    xd = (xh[0] * ds[0] + xh[1] * ds[1]) + xh[2] * ds[2]
    t2, k2 = t * t, kk * kk
    rad, t4 = xd * t2, t2 * t2
    sq = [h * h for h in xh]
    out = []
    for c in range(3):
        jd = kk * (ds[c] - xh[c] * xd) + xh[c] * rad
        jd2 = jd * jd
        jj = k2 * (sq[(c + 1) % 3] + sq[(c + 2) % 3]) + sq[c] * t4
        out.append(var_t * jd2 + var_r * (jj - jd2 / dn))
    var = Fl(torch.cat([w.v for w in out], -1), torch.cat([w.e for w in out], -1)).where(outside, diag)
    return mu, var


def kernel_bounds(z, rays, L, r2, dn, mode="gaussian", path="direct", stored_bf16=False):
    """-> dict: feat, mu (Fl; feat (N,S,6L) in the reference's column order), var (Fl), inside (N,S) bool: the metric mean is in the ball.
    `stored_bf16`: feat and mu are read from a bf16 dump."""
    mu, var = fl_gaussian(z, rays, r2, dn, mode)
    N, S = mu.v.shape[:2]
    sins, coss = [], []
    if path == "direct":
        for l in range(L):
            arg = mu.scaled(2.0 ** l)
            att = fl_exp(var.scaled(-0.5 * 4.0 ** l))
            sins.append(fl_sin(arg) * att)
            coss.append(fl_cos(arg) * att)
    else:
        s, c, att = fl_sin(mu), fl_cos(mu), fl_exp(var.scaled(-0.5))
        for l in range(L):
            sins.append(s * att)
            coss.append(c * att)
            s2 = s.scaled(2.0)
            s, c = s2 * c, fma(s2.scaled(-1.0), s, Fl(1.0))
            a2 = att * att
            att = a2 * a2
    v = torch.stack([torch.cat((a.v, b.v), -1) for a, b in zip(sins, coss)], 2).reshape(N, S, 6 * L)
    e = torch.stack([torch.cat((a.e, b.e), -1) for a, b in zip(sins, coss)], 2).reshape(N, S, 6 * L)
    feat = Fl(v, e)
    if stored_bf16:
        feat, mu = feat.stored_bf16(), mu.stored_bf16()
    x = rays[:, None, :3].double() + cone_moments(z)[0][..., None] * rays[:, None, 3:6].double()
    return {"feat": feat, "mu": mu, "var": var, "inside": x.norm(dim=-1) <= 1}


# ------------------------------------------------------------------------------------------------ the comparator
def compare(bounds, feat, mu, twin=None):
    """feat (N,S,6L), mu (N,S,3): what a kernel wrote (any float dtype, CPU).  twin = (feat, mu) of the contract = 1 run on the same
    inputs, or None.  -> {"feat": max(err / tol), "mu": max(err / tol), "inside-bits": elements of inside-ball frusta that differ from
    the twin's bits (0 without a twin)}; a non-finite output counts as inf."""
    rep = {}
    for name, got in (("feat", feat), ("mu", mu)):
        b = bounds[name]
        g = got.double().reshape(b.v.shape)
        ratio = (g - b.v).abs() / b.e
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        rep[name] = float(ratio.max())
    rep["inside-bits"] = 0.0
    if twin is not None:
        ins = bounds["inside"]
        for got, tw in ((feat, twin[0]), (mu, twin[1])):
            a, b = got.float().reshape(ins.shape + (-1,))[ins], tw.float().reshape(ins.shape + (-1,))[ins]
            rep["inside-bits"] += float((a.view(torch.int32) != b.view(torch.int32)).sum())
    return rep


def assert_compare(what, rep):
    bad = {k: v for k, v in rep.items() if not v <= (0.0 if k == "inside-bits" else 1.0)}
    assert not bad, "%s: beyond the bound in %s" % (what, ", ".join("%s (%.3g)" % kv for kv in sorted(bad.items())))
