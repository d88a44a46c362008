"""The regulariser kernels of nerf_amd/csrc/sample_kernels.hip -- distortion_loss_kernel<0|1>, distortion_loss_backward_kernel<0|1>,
interlevel_loss_kernel, interlevel_loss_backward_kernel -- for the tests: fp64 specifications, a bound for every element of every output,
a torch emulation of each kernel (its CPU twin, which also carries the planted faults), the shared input generator and the check
functions that tests/test_regularizer_ref_host.py runs over the emulation and tests/test_gpu_regularizers.py over nerf_amd.ops.
Plain torch on whatever device the inputs live on; nothing of the package is imported.

CONSTANTS  u = 2^-24 (one fp32 rounding, relative), eps = 2^-53 (one fp64 operation, sqrt and division included), 2^-150 (half the
smallest fp32 subnormal: the absolute part of a cast that lands below 2^-126).  cast(x, E) = u |x| + (1 + u) E (+ 2^-150 where
|x| + E < 2^-125) is the bound of an fp32 store of a value whose fp64 error is E.  EM = (2 M + 8) eps stands for a fused fp64 sum of M
terms in the kernel's order AND the specification's own sum of the same terms in torch's order; it always multiplies the sum of the
terms' magnitudes, never the magnitude of the sum.

DISTORTION.  dist_stage forms, in fp32 from the fp32 inputs, c_i = (t_i + t_i+1) / 2, d_i = t_i+1 - t_i and (mode 0) a_i = (w_i +
w_i+1) / 2; the specification forms the same three in fp32 (so they are bit-equal on both sides and their chain rule, the two-tap
scatter with the exact factors 1/2 and +-1, is applied in fp64), everything after in fp64, gradients by autograd on the fp64 leaves.
The kernels' operation list, in order, with x_kj = c_k - c_j exact (a difference of two fp32 numbers is an fp64 number):
  1. d_kj = fl32(c_k - c_j): e_kj = |d_kj - x_kj| is COMPUTED, not bounded -- it is 0 wherever the subtraction is exact (Sterbenz:
     c_j / 2 <= c_k <= 2 c_j, every pair of a clustered row), at most u |x_kj| elsewhere; sign and zero-ness are always exact, so
     s_kj = sgn(d_kj) carries no error.
  2. the fused fp64 sums over j.  D_k = sum a_j |d_kj|: eD_k = sum |a_j| e_kj + EM sum |a_j x_kj|.  R2_k = sum d_kj^2: relative
     rho_k = sum (2 |x_kj| e_kj + e_kj^2) / R2_k + EM.  Cs_k = sum d_kj: sum e_kj + EM sum |x_kj|.  Sg_k = sum a_j s_kj: EM sum |a_j s_kj|.
  3. mode 0, pass 1: r = sqrt(R2), u_k = a_k / r_k, q_k = a_k D_k / (r_k R2_k):  du_k = |u_k| (rho_k / 2 + 4 eps),
     dq_k = |q_k| (3 rho_k / 2 + 8 eps) + |a_k| eD_k / (r_k R2_k).
  4. mode 0, pass 2:  E_k = sum u_j |d_kj|: dE_k = sum (du_j |x_kj| + |u_j| e_kj) + EM sum |u_j x_kj|;  T_k = sum u_j s_kj: dT_k = sum
     du_j |s_kj| + EM sum |u_j s_kj|;  V_k = sum q_j d_kj: dV_k = sum (dq_j |x_kj| + |q_j| e_kj) + EM sum |q_j x_kj|.
  5. ga_k = kP (D_k / r_k + E_k) + kQ 2 d_k a_k:  |kP| (eD_k / r_k + (D_k / r_k)(rho_k / 2 + 4 eps) + dE_k + 4 eps (D_k / r_k + |E_k|))
     + 6 eps |kQ 2 d_k a_k|.   Mode 1: ga_k = kP 2 D_k + kQ 2 d_k a_k: 2 |kP| eD_k + 6 eps (both magnitudes).
  6. gc_k = kP (((u_k Sg_k + a_k T_k) - q_k Cs_k) - V_k) -- the two cancellations of mode 0: the four products keep their own errors
     du |Sg| + |u| dSg + |a| dT + dq |Cs| + |q| dCs + dV, and the three additions cost 6 eps (|u Sg| + |a T| + |q Cs| + |V|), the SUM of
     the magnitudes (with two intervals the four terms cancel exactly and this is all that is left on either side).
     Mode 1: gc_k = kP 2 a_k Sg_k: 2 |kP a_k| dSg_k + 4 eps |gc_k|.     gd_k = kQ a_k^2: 4 eps |gd_k|.
  7. the two-tap scatter: d_t[k] = (gc_k / 2 - gd_k) + (gc_k-1 / 2 + gd_k-1), mode 0 d_w[k] = ga_k / 2 + ga_k-1 / 2 (the lower part by
     shuffle, by `carry` across lane 63, column M from the carry when M % 128 == 0: data movement, exact): the parts' errors plus
     3 eps times the sum of the four (two) magnitudes; then the store, cast().   Mode 1 d_w[k] = ga_k.
  kP = g scale cP, kQ = g scale cQ: g scale is exact in fp64 (two fp32 factors), cP and cQ cost two roundings each, inside the eps terms.
  The loss: sum_n sum_k a_k D_k (/ r_k) inherits step 2 (and rho_k / 2 of r_k), sum d_k a_k^2 is exact to 3 eps; lane, block and grid
  reductions in fp64 of non-negative terms: (M + N / 1024 + 64) 2 eps of the value; then the store.
  EXACT: an element all of whose terms are exact zeros has E = 0 and want = 0, so tol = 0: equality.  A ray whose centres coincide has
  R2 = 0: mode 0 gives NaN in every gradient column of THAT ray and in the loss, nothing else; mode 1 gives exact zeros.

INTERLEVEL.  The specification sums, for every fine interval, the proposal weights the overlap mask selects (interlevel_ref.brute_bounds:
no prefix sum, so no cancellation of its own, and an empty selection is an exact 0); the gradient is autograd through that mask, a direct
sum over the fine intervals [i0, i1) of one proposal interval.  The kernels:
  1. c = exclusive fp64 prefix sum of w_prop by a 64-lane wave scan (six levels) plus a carry per block: c_j passes 7 + j / 64 additions,
     error (7 + j / 64) eps cabs_j with cabs the prefix sum of |w_prop|  (this is the scan order against the exact sum; torch.cumsum's
     sequential order would have j eps cabs_j).
  2. bound_i = c[hi] - c[lo], the `total - prefix` difference: eb_i = eps ((7 + hi/64) cabs_hi + (7 + lo/64) cabs_lo + 2 |b_i|) +
     (K + 2) eps babs_i (the specification's own sum); hi == lo (a closed proposal span that the interval lies outside) is c - c of ONE
     entry: exactly 0.  bounds_out: cast(b_i, eb_i).
  3. the loss term relu(w - b)^2 / (w + 1e-8) in fp64: (2 relu(w - b) eb + eb^2) / (w + 1e-8) + 6 eps term; lane, block and grid
     reductions (M / 64 + N / 1024 + 32) 2 eps of the sum; times |scale|; the store.
  4. f_i = -2 relu(w_i - b_i) / (w_i + 1e-8): ef_i = 2 eb_i / (w_i + 1e-8) (0 where w_i - b_i < -eb_i: both sides take the zero branch)
     + 4 eps |f_i|.
  5. F = prefix sum of f by the same scan, d_w_prop[j] = g scale (F[i1] - F[i0]): |g scale| (sum_[i0,i1) ef_i + eps ((7 + i1/64) Fabs_i1 +
     (7 + i0/64) Fabs_i0) + (M + 4) eps sum_[i0,i1) |f_i|); i1 <= i0 stores the constant 0: exact.  Then the store.

TIGHTNESS is shown by the emulation's share of each bound and by the planted faults (tests/test_regularizer_ref_host.py prints both)."""
import numpy as np
import torch

import interlevel_ref as R
from ray_stages_ref import worst as _worst

F32, F64 = torch.float32, torch.float64
INF = float("inf")
U = 2.0 ** -24
EPS64 = 2.0 ** -53
HALF_ETA = 2.0 ** -150
POISON = -7.0
CHUNK = 1 << 25                                            # elements of an (n, M, M) / (n, M, K) intermediate (the issue allows 2^26)

DIST_FAMILIES = {0: ("uniform", "peaked", "clustered", "unsorted", "degenerate"), 1: ("uniform", "peaked", "clustered", "degenerate")}
IL_FAMILIES = ("uniform", "peaked", "clustered", "ties", "degenerate")
GS = (1.0, 0.37, -2.5)                                     # upstream gradients (0-dim device tensors in the calls)
SCALES = (1.0, 0.25, 3.0)
HOST_S = (2, 3, 4, 64, 65, 66, 128, 129, 130, 257)
HOST_IL_SHAPES = R.HOST_SHAPES


def f32c(v):
    """a Python float argument as the kernel receives it"""
    return float(np.float32(v))


def pick(values, *keys):
    """a deterministic choice that cycles through `values` as the keys vary (the g and scale of a case)"""
    return values[sum(int(k) * (i + 1) for i, k in enumerate(keys)) % len(values)]


# ------------------------------------------------------------------------------------------------ the comparator
def worst(got, want, tol):
    """max over every element of |got - want| / tol (ray_stages_ref.worst: inf for any error against a zero tolerance, for a non-finite
    got or tol), with the NaN pattern matched exactly: got must be NaN where and only where the specification is NaN"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    tol = torch.as_tensor(tol).detach().double().cpu().expand_as(want)
    assert got.shape == want.shape, "shape %s, expected %s" % (tuple(got.shape), tuple(want.shape))
    nan = torch.isnan(want)
    if bool((torch.isnan(got) != nan).any()):
        return INF
    if bool(nan.all()):
        return 0.0
    return _worst(got[~nan], want[~nan], tol[~nan])


def exact_mismatches(got, want, tol):
    """the exact statements, counted: elements whose bound is 0 (equality) and differ, plus NaN-pattern mismatches"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    tol = torch.as_tensor(tol).detach().double().cpu().expand_as(want)
    nan = torch.isnan(want)
    return int((torch.isnan(got) != nan).sum()) + int(((tol == 0) & ~nan & ~(got == want)).sum())


def cast_tol(want, err):
    want, err = want.abs(), err
    tol = U * want + (1.0 + U) * err
    small = (want + err > 0) & (want + err < 2.0 ** -125)
    return torch.where(small, tol + HALF_ETA, tol)


# ------------------------------------------------------------------------------------------------ the input generator
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _bump_params(N, g):
    return 3.0 + 2.0 * torch.rand(N, 1, generator=g, dtype=F64), 0.05 + 0.10 * torch.rand(N, 1, generator=g, dtype=F64)


def _bump(x, mu, sig):
    """a narrow bump in depth: at least ten decades from its top to the smallest value kept, exact zeros beyond (below 1e-12)"""
    w = torch.exp(-0.5 * ((x.double() - mu) / sig) ** 2)
    return torch.where(w >= 1e-12, w, torch.zeros_like(w)).float()


def _special_rows(w, skip=()):
    """ray 0 one-hot, ray 1 all zero (batches of at least four rays)"""
    if w.shape[0] >= 4:
        if 0 not in skip:
            w[0] = 0.0
            w[0, w.shape[1] // 3] = 1.0
        w[1] = 0.0
    return w


def _clustered_edges(N, S, mu, sig, g):
    """S edges per row by inverse CDF from the peaked histogram over 64 bins of [2, 6], sorted, with a run of three bit-equal edges in the
    lower half and a run of two in the upper half of every row (S >= 6; S = 4, 5: one run of two; below that none, a run would make the
    whole row coincide): zero-width intervals, and tied centres inside the run of three"""
    grid = torch.linspace(2.0, 6.0, 65)
    hist = _bump((grid[:-1] + grid[1:])[None, :].expand(N, -1) / 2, mu, sig).double()
    cdf = torch.cat((torch.zeros(N, 1, dtype=F64), torch.cumsum(hist, -1) / hist.sum(-1, keepdim=True)), -1)
    u = torch.rand(N, S, generator=g, dtype=F64) * (1 - 1e-9)
    idx = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True).clamp(1, 64)
    c0, c1 = torch.gather(cdf, 1, idx - 1), torch.gather(cdf, 1, idx)
    t = (grid.double()[idx - 1] + (u - c0) / (c1 - c0) * (4.0 / 64)).float()
    t = torch.sort(t, dim=-1)[0]
    rows = torch.arange(N)
    if S >= 6:
        p3 = torch.randint(0, S // 2 - 2, (N,), generator=g)
        p2 = S // 2 + torch.randint(0, S - 1 - S // 2, (N,), generator=g)
        t[rows, p3 + 1] = t[rows, p3]
        t[rows, p3 + 2] = t[rows, p3]
        t[rows, p2 + 1] = t[rows, p2]
    elif S >= 4:
        t[:, 2] = t[:, 1]
    return t.contiguous()


def old_dist_inputs(N, S, mode, seed):
    """tests/test_gpu_distortion.py _inputs, the `uniform` family (the host test asserts they are the same)"""
    g = _gen(seed)
    t = 2.0 + 4.0 * torch.rand(N, S, generator=g)
    if mode == 1:
        t = torch.sort(t, dim=-1)[0]
    w = torch.rand(N, S if mode == 0 else S - 1, generator=g)
    return w, t


def _centres(t):
    return (t[:, :-1] + t[:, 1:]) / 2


def dist_inputs(family, N, S, mode, seed):
    """fp32 (w, t) of nerf_amd_distortion_loss: w (N, S) in mode 0, (N, S - 1) in mode 1; t (N, S).  `degenerate` has at least 9 rays"""
    assert family in DIST_FAMILIES[mode], (family, mode)
    g = _gen(seed)
    if family in ("uniform", "degenerate"):
        N = max(N, 9) if family == "degenerate" else N
        w, t = old_dist_inputs(N, S, mode, seed)
        if family == "degenerate":
            t[2] = 3.0                                                               # ray 2: every centre coincides
        return w.contiguous(), t.contiguous()
    mu, sig = _bump_params(N, g)
    if family == "peaked":
        t = torch.sort(2.0 + 4.0 * torch.rand(N, S, generator=g), dim=-1)[0]
        w = _special_rows(_bump(t if mode == 0 else _centres(t), mu, sig))
        return w.contiguous(), t.contiguous()
    t = _clustered_edges(N, S, mu, sig, g)
    w = _bump(t if mode == 0 else _centres(t), mu, sig)
    if family == "unsorted":
        perm = torch.argsort(torch.rand(N, S, generator=g), dim=-1)
        t, w = torch.gather(t, 1, perm), torch.gather(w, 1, perm)
    return w.contiguous(), t.contiguous()


def _normalised(w):
    return (w.double() / w.double().sum(-1, keepdim=True).clamp_min(1e-300)).float()


def il_inputs(family, N, M, K, open_form, seed):
    """fp32 (w (N, M), t (N, M + 1), w_prop (N, K), t_prop (N, Kp)) of nerf_amd_interlevel_loss, Kp = K (open form) or K + 1"""
    assert family in IL_FAMILIES, family
    if family in ("uniform", "degenerate"):
        N = max(N, 9) if family == "degenerate" else N
        w, t, w_prop, t_prop = R.make_inputs(N, M, K, open_form, False, seed)
        if family == "degenerate":
            t[2] = t[2, M // 2]                                                      # ray 2: M zero-width fine intervals on one depth
        return w, t.contiguous(), w_prop, t_prop
    g = _gen(seed)
    Kp = K if open_form else K + 1
    mu, sig = _bump_params(N, g)
    mu2, sig2 = mu + 0.3 * sig, 1.3 * sig

    def weights(t, t_prop):
        pc = t_prop if open_form else _centres(t_prop)
        return _normalised(_bump(_centres(t), mu, sig)), _normalised(_bump(pc, mu2, sig2))

    def peaked(n):
        t = torch.sort(2.0 + 4.0 * torch.rand(n, M + 1, generator=g), dim=-1)[0]
        t_prop = torch.sort(1.5 + 5.0 * torch.rand(n, Kp, generator=g), dim=-1)[0]
        return t, t_prop

    if family == "peaked":
        t, t_prop = peaked(N)
    elif family == "clustered":
        t, t_prop = _clustered_edges(N, M + 1, mu, sig, g), _clustered_edges(N, Kp, mu2, sig2, g)
    else:                                                                            # ties: even rays on peaked, odd rays on clustered rows
        t, t_prop = peaked(N)
        tc, tpc = _clustered_edges(N, M + 1, mu, sig, g), _clustered_edges(N, Kp, mu2, sig2, g)
        t[1::2], t_prop[1::2] = tc[1::2], tpc[1::2]
        if M >= 2:                                                                   # reaching below the first and above the last proposal edge
            t[:, 0] = t_prop[:, 0] - 0.25
            t[:, -1] = t_prop[:, -1] + 0.25
            picked = t_prop[:, ::2]
            if picked.shape[1] > M - 1:
                picked = picked[:, torch.linspace(0, picked.shape[1] - 1, M - 1).round().long()]
            t[:, 1: 1 + picked.shape[1]] = picked                                    # fine edges that ARE proposal edges, bit for bit
        t = torch.sort(t, dim=-1)[0]
    w, w_prop = weights(t, t_prop)
    if family == "peaked":
        w = _special_rows(w)
        if N >= 4:
            w_prop[1] = 0.0
    return w.contiguous(), t.contiguous(), w_prop.contiguous(), t_prop.contiguous()


# ------------------------------------------------------------------------------------------------ distortion: specification and bounds
def dist_coeffs(mode, N, M):
    return (1.0 / (float(N) * M * M), 1.0 / (3.0 * N * M)) if mode == 0 else (1.0 / float(N), 1.0 / (3.0 * N))


def _staged(w, t, mode):
    """what dist_stage forms in fp32 from the fp32 inputs, widened: centres, (mode 0: averaged) weights, widths; and the fp32 centres"""
    c32 = (t[:, :-1] + t[:, 1:]) / 2.0
    a32 = (w[:, :-1] + w[:, 1:]) / 2.0 if mode == 0 else w
    return c32.double(), a32.double(), (t[:, 1:] - t[:, :-1]).double(), c32


def _two_tap(h, l):
    """column k = h_k + l_k-1 over M + 1 columns (h_M = 0, l_-1 = 0)"""
    z = torch.zeros_like(h[:, :1])
    return torch.cat((h, z), 1) + torch.cat((z, l), 1)


def _dist_chunk(w, t, mode, kP, kQ, M):
    """one chunk of rays -> (sum P, sum Q, error of sum P) and the per-column gradients with their fp64 errors"""
    c, a, dl, c32 = _staged(w, t, mode)
    cl, al, dll = (x.clone().requires_grad_(True) for x in (c, a, dl))
    dist = (cl[:, :, None] - cl[:, None, :]).abs()
    if mode == 0:
        dist = dist / torch.sqrt((dist ** 2).sum(-1, keepdim=True))
    P, Q = (al[:, :, None] * al[:, None, :] * dist).sum(), (dll * al * al).sum()
    ga, gc, gd = torch.autograd.grad(kP * P + kQ * Q, (al, cl, dll))
    del dist
    # ---- the bound (see the module docstring; every quantity is a function of the element's own terms)
    EM = (2 * M + 8) * EPS64
    x = c[:, :, None] - c[:, None, :]
    e = ((c32[:, :, None] - c32[:, None, :]).double() - x).abs()
    ax, s = x.abs(), (x != 0).double()
    aa = a.abs()[:, None, :]
    D, Dabs = (a[:, None, :] * ax).sum(-1), (aa * ax).sum(-1)
    eD = (aa * e).sum(-1) + EM * Dabs
    Sg, dSg = (a[:, None, :] * torch.sign(x)).sum(-1), EM * (aa * s).sum(-1)
    kp, kq = abs(kP), abs(kQ)
    magQ = kq * (2.0 * dl * a).abs()
    e_gd, m_gd = 4 * EPS64 * kq * a * a, kq * a * a
    if mode == 1:
        e_ga = 2 * kp * eD + 6 * EPS64 * (2 * kp * Dabs + magQ)
        m_gc = 2 * kp * (a * Sg).abs()
        e_gc = 2 * kp * a.abs() * dSg + 4 * EPS64 * m_gc
        errP = (a.abs() * eD).sum()
    else:
        R2 = (x * x).sum(-1)
        rr = torch.sqrt(R2)
        rho = (2 * ax * e + e * e).sum(-1) / R2 + EM
        u, q = a / rr, a * D / (rr * R2)
        du = u.abs() * (rho / 2 + 4 * EPS64)
        dq = q.abs() * (1.5 * rho + 8 * EPS64) + a.abs() * eD / (rr * R2)
        uj, qj, duj, dqj = u.abs()[:, None, :], q.abs()[:, None, :], du[:, None, :], dq[:, None, :]
        E = (u[:, None, :] * ax).sum(-1)
        dE = (duj * ax + uj * e).sum(-1) + EM * (uj * ax).sum(-1)
        T, dT = (u[:, None, :] * torch.sign(x)).sum(-1), (duj * s).sum(-1) + EM * (uj * s).sum(-1)
        V, dV = (q[:, None, :] * x).sum(-1), (dqj * ax + qj * e).sum(-1) + EM * (qj * ax).sum(-1)
        Cs, dCs = x.sum(-1), e.sum(-1) + EM * ax.sum(-1)
        e_ga = kp * (eD / rr + (D / rr) * (rho / 2 + 4 * EPS64) + dE + 4 * EPS64 * (D / rr + E.abs())) + 6 * EPS64 * magQ
        m_gc = kp * ((u * Sg).abs() + (a * T).abs() + (q * Cs).abs() + V.abs())
        e_gc = kp * (du * Sg.abs() + u.abs() * dSg + a.abs() * dT + dq * Cs.abs() + q.abs() * dCs + dV) + 6 * EPS64 * m_gc
        errP = (a.abs() * (eD / rr + (D / rr) * (rho / 2 + 4 * EPS64))).sum()
    m_ga = ga.abs() + e_ga
    d_t = _two_tap(0.5 * gc - gd, 0.5 * gc + gd)
    e_t = _two_tap(0.5 * e_gc + e_gd, 0.5 * e_gc + e_gd) + 3 * EPS64 * _two_tap(0.5 * m_gc + m_gd, 0.5 * m_gc + m_gd)
    if mode == 0:
        d_w = _two_tap(0.5 * ga, 0.5 * ga)
        e_w = _two_tap(0.5 * e_ga, 0.5 * e_ga) + 3 * EPS64 * _two_tap(0.5 * m_ga, 0.5 * m_ga)
    else:
        d_w, e_w = ga, e_ga
    return P.detach(), Q.detach(), errP, d_w, cast_tol(d_w, e_w), d_t, cast_tol(d_t, e_t)


def dist_ref(w, t, mode, g=1.0, scale=1.0):
    """fp32 inputs on any device -> {"loss": (want, tol), "d_w": (want, tol), "d_t": (want, tol)}, fp64, for upstream gradient g and
    `scale`; the loss is not multiplied by g"""
    w, t = w.detach().float(), t.detach().float()
    N, S = t.shape
    M = S - 1
    gs = float(np.float32(g)) * f32c(scale)
    cP, cQ = dist_coeffs(mode, N, M)
    step = max(1, CHUNK // (M * M))
    d_w, t_w = torch.empty_like(w, dtype=F64), torch.empty_like(w, dtype=F64)
    d_t, t_t = torch.empty_like(t, dtype=F64), torch.empty_like(t, dtype=F64)
    P = Q = eP = torch.zeros((), dtype=F64, device=t.device)
    for s0 in range(0, N, step):
        sl = slice(s0, s0 + step)
        p, q, ep, d_w[sl], t_w[sl], d_t[sl], t_t[sl] = _dist_chunk(w[sl], t[sl], mode, gs * cP, gs * cQ, M)
        P, Q, eP = P + p, Q + q, eP + ep
    sc = f32c(scale)
    loss = (P * cP + Q * cQ) * sc
    depth = (M + N // 1024 + 64) * 2 * EPS64
    tol = cast_tol(loss, abs(sc) * (cP * eP + depth * (cP * P.abs() + cQ * Q.abs())))
    return {"loss": (loss, tol), "d_w": (d_w, t_w), "d_t": (d_t, t_t)}


# ------------------------------------------------------------------------------------------------ interlevel: specification and bounds
def _excl(x):
    return torch.cat((torch.zeros_like(x[:, :1]), torch.cumsum(x, -1)), -1)


def il_ref(w, t, w_prop, t_prop, g=1.0, scale=1.0):
    """fp32 inputs on any device -> {"loss", "bounds", "d_w_prop"}: (want, tol) each, fp64"""
    w, t, w_prop, t_prop = (v.detach().double() for v in (w, t, w_prop, t_prop))
    N, M, K = w.shape[0], w.shape[1], w_prop.shape[1]
    sc = f32c(scale)
    gs = float(np.float32(g)) * sc
    step = max(1, CHUNK // (M * K))
    bounds, t_b = torch.empty_like(w), torch.empty_like(w)
    grad, t_g = torch.empty_like(w_prop), torch.empty_like(w_prop)
    loss = e_loss = torch.zeros((), dtype=F64, device=w.device)
    depth = (M // 64 + N // 1024 + 32) * 2 * EPS64
    for s0 in range(0, N, step):
        sl = slice(s0, s0 + step)
        wn, tn, en = w[sl], t[sl], R._edges(w_prop[sl], t_prop[sl])
        p = w_prop[sl].clone().requires_grad_(True)
        mask = ((tn[:, :-1, None] < en[:, None, 1:]) & (tn[:, 1:, None] >= en[:, None, :-1])).double()
        b = (mask * p[:, None, :]).sum(-1)
        part = R.loss_from_bounds(wn, b, 1.0)
        grad[sl] = gs * torch.autograd.grad(part, p)[0]
        b, p = b.detach(), p.detach()
        # ---- the bound
        cnt = torch.searchsorted(en.contiguous(), tn.contiguous(), right=True)
        lo, hi = (cnt[:, :-1] - 1).clamp(min=0), cnt[:, 1:].clamp(max=K)
        cabs = _excl(p.abs())
        eb = EPS64 * ((7 + hi // 64) * torch.gather(cabs, 1, hi) + (7 + lo // 64) * torch.gather(cabs, 1, lo) + 2 * b.abs()) \
            + (K + 2) * EPS64 * (mask * p.abs()[:, None, :]).sum(-1)
        eb = torch.where(hi == lo, torch.zeros_like(eb), eb)
        bounds[sl], t_b[sl] = b, cast_tol(b, eb)
        d = torch.relu(wn - b)
        term = d * d / (wn + R.EPS)
        loss = loss + part.detach()
        e_loss = e_loss + ((2 * d * eb + eb * eb) / (wn + R.EPS) + 6 * EPS64 * term).sum() + depth * term.sum()
        f = 2 * d / (wn + R.EPS)
        ef = torch.where(wn - b < -eb, torch.zeros_like(eb), 2 * eb / (wn + R.EPS)) + 4 * EPS64 * f
        Fabs = _excl(f)
        i1 = torch.searchsorted(tn[:, :M].contiguous(), en[:, 1:].contiguous(), right=False)
        i0 = torch.searchsorted(tn[:, 1:].contiguous(), en[:, :-1].contiguous(), right=False)
        rng = (mask * (ef + (M + 4) * EPS64 * f)[:, :, None]).sum(1)
        eg = abs(gs) * (rng + EPS64 * ((7 + i1 // 64) * torch.gather(Fabs, 1, i1.clamp(max=M)) + (7 + i0 // 64) * torch.gather(Fabs, 1, i0.clamp(max=M))))
        eg = torch.where(i1 <= i0, torch.zeros_like(eg), eg + 2 * EPS64 * grad[sl].abs())
        t_g[sl] = cast_tol(grad[sl], eg)
    loss = loss * sc
    return {"loss": (loss, cast_tol(loss, abs(sc) * e_loss)), "bounds": (bounds, t_b), "d_w_prop": (grad, t_g)}


# ------------------------------------------------------------------------------------------------ the emulation (and the planted faults)
DIST_FAULTS = ("sgn0_plus", "colM_unwritten", "no_handover", "carry_kept", "q_term_w", "third_dropped_dt", "uq_fp32", "pair_sums_fp32", "g_one", "scale_twice")
IL_FAULTS = ("g_one", "scale_twice", "lo_unclamped", "hi_count_lt", "open_last_depth", "F_carry_dropped", "no_eps", "cprefix_fp32", "F_prefix_fp32")


def _wave_scan(v):
    """device_common.h wave_incl_scan on (..., 64) doubles: the inclusive scan in the kernel's order of additions"""
    shape = v.shape
    for sh in (1, 2, 4, 8):                                                          # row_shr:sh inside each row of 16 lanes
        rows = v.reshape(shape[:-1] + (4, 16))
        s = torch.zeros_like(rows)
        s[..., sh:] = rows[..., :-sh]
        v = (rows + s).reshape(shape)
    b = torch.zeros_like(v)                                                          # row_bcast:15, rows 1 and 3
    b[..., 16:32] = v[..., 15:16]
    b[..., 48:64] = v[..., 47:48]
    v = v + b
    b = torch.zeros_like(v)                                                          # row_bcast:31, rows 2 and 3
    b[..., 32:64] = v[..., 31:32]
    return v + b


def wave_prefix(x, drop_carry=False):
    """(N, L) doubles -> (N, L + 1): the exclusive prefix sum as il_stage forms it, a wave scan per 64 columns plus the carried total"""
    N, L = x.shape
    nb = (L + 63) // 64
    xp = torch.cat((x, x.new_zeros(N, nb * 64 - L)), 1).reshape(N, nb, 64)
    sc = _wave_scan(xp)
    out, carry = [x.new_zeros(N, 1)], x.new_zeros(N)
    for b in range(nb):
        v = sc[:, b] + carry[:, None]
        out.append(v)
        carry = torch.zeros_like(carry) if drop_carry else v[:, 63]
    return torch.cat(out, 1)[:, : L + 1]


class Emulation:
    """Each kernel in torch: the fp32 roundings where the kernel has them (the staged row, d = c_k - c_j, the stores), fp64 elsewhere,
    the backward by the closed forms of the comment above dist_coeffs and by the F prefix.  `faults` plants single-term changes.
    `cap` is the grid cap in workgroups of four waves (the device's is 2048; the host runs with 1 so that rays 4, 5, ... are second trips)"""

    def __init__(self, faults=(), cap=1):
        assert set(faults) <= set(DIST_FAULTS) | set(IL_FAULTS), faults
        self.faults, self.cap = tuple(faults), cap

    def _gs(self, g, scale):
        g = 1.0 if "g_one" in self.faults else float(torch.as_tensor(g).float())
        return g * f32c(scale) * (f32c(scale) if "scale_twice" in self.faults else 1.0)

    # ---- distortion
    def _dist_rows(self, w, t, mode, kP, kQ):
        """(ga, gc, gd, P row sums, Q row sums) of a chunk of rays"""
        f = self.faults
        M = t.shape[1] - 1
        c, a, dl, c32 = _staged(w, t, mode)
        d = (c32[:, :, None] - c32[:, None, :]).double()                             # fl32(c_k - c_j), [n, k, j]
        ad, s = d.abs(), torch.sign(d)
        if "sgn0_plus" in f:
            s = torch.where((d == 0) & ~torch.eye(M, dtype=torch.bool, device=d.device), torch.ones_like(s), s)
        aj = a[:, None, :]
        D = (aj.float() * ad.float()).sum(-1).double() if "pair_sums_fp32" in f else (aj * ad).sum(-1)
        aQ = w[:, :M].double() if (mode == 0 and "q_term_w" in f) else a
        gd = kQ * (aQ * aQ) * (3.0 if "third_dropped_dt" in f else 1.0)
        if mode == 1:
            Sg = (aj * s).sum(-1)
            return kP * (2.0 * D) + kQ * (2.0 * dl * aQ), kP * (2.0 * a * Sg), gd, (a * D).sum(-1), (dl * a * a).sum(-1)
        R2 = (d * d).sum(-1)
        rr = torch.sqrt(R2)
        u, q = a / rr, a * D / (rr * R2)
        uj, qj = (u.float().double(), q.float().double()) if "uq_fp32" in f else (u, q)
        uj, qj = uj[:, None, :], qj[:, None, :]
        E, Sg, T, V, Cs = (uj * ad).sum(-1), (aj * s).sum(-1), (uj * s).sum(-1), (qj * d).sum(-1), d.sum(-1)
        ga = kP * (D / rr + E) + kQ * (2.0 * dl * aQ)
        gc = kP * (((u * Sg + a * T) - q * Cs) - V)
        return ga, gc, gd, (a * D / rr).sum(-1), (dl * a * a).sum(-1)

    def _dist_all(self, w, t, mode, kP, kQ):
        N, M = t.shape[0], t.shape[1] - 1
        step = max(1, CHUNK // (M * M))
        parts = [self._dist_rows(w[s0:s0 + step], t[s0:s0 + step], mode, kP, kQ) for s0 in range(0, N, step)]
        return [torch.cat(p, 0) for p in zip(*parts)]

    def distortion_loss(self, w, t, mode, scale):
        N, M = t.shape[0], t.shape[1] - 1
        cP, cQ = dist_coeffs(mode, N, M)
        _, _, _, P, Q = self._dist_all(w.float(), t.float(), mode, 1.0, 1.0)
        return ((P.sum() * cP + Q.sum() * cQ) * f32c(scale)).float()

    def distortion_backward(self, g, w, t, mode, scale, need=(True, True)):
        f = self.faults
        N, M = t.shape[0], t.shape[1] - 1
        cP, cQ = dist_coeffs(mode, N, M)
        gs = self._gs(g, scale)
        ga, gc, gd, _, _ = self._dist_all(w.float(), t.float(), mode, cP * gs, cQ * gs)
        z = torch.zeros_like(ga[:, :1])

        def scatter(h, l):
            below = torch.cat((z, l), 1)                                             # column k takes l_k-1: shuffle, or `carry` across lane 63
            if "no_handover" in f:
                below[:, 64::64] = 0.0
            if "carry_kept" in f and M % 128 == 0:                                   # the wave's previous ray left l_M-1 in the carry
                stride = 4 * min((N + 3) // 4, self.cap)
                below[stride:, 0] = below[stride:, 0] + l[:-stride, M - 1]
            out = (torch.cat((h, z), 1) + below).float()
            if "colM_unwritten" in f and M % 128 == 0:
                out[:, M] = POISON
            return out

        d_t = scatter(0.5 * gc - gd, 0.5 * gc + gd) if need[1] else None
        d_w = None
        if need[0]:
            d_w = scatter(0.5 * ga, 0.5 * ga) if mode == 0 else ga.float()
        return d_w, d_t

    # ---- interlevel
    def _il_stage(self, t, w_prop, t_prop):
        f = self.faults
        K = w_prop.shape[1]
        e = R._edges(w_prop, t_prop)
        if "open_last_depth" in f and t_prop.shape[1] == K:
            e = torch.cat((t_prop, t_prop[:, -1:]), 1)
        c = _excl(w_prop.float()).double() if "cprefix_fp32" in f else wave_prefix(w_prop.double())
        cnt = torch.searchsorted(e.contiguous(), t.contiguous(), right=True)         # count_le
        ch = torch.searchsorted(e.contiguous(), t.contiguous(), right=False)[:, 1:] if "hi_count_lt" in f else cnt[:, 1:]
        lo = cnt[:, :-1] - 1
        lo = lo % (K + 1) if "lo_unclamped" in f else lo.clamp(min=0)                # (the fault reads the entry before the row: here the last)
        b = torch.gather(c, 1, ch.clamp(max=K)) - torch.gather(c, 1, lo)
        return e, b

    def interlevel_loss(self, w, t, w_prop, t_prop, scale):
        """-> (loss fp32 0-dim, bounds fp32)"""
        w, t, w_prop, t_prop = (v.float() for v in (w, t, w_prop, t_prop))
        _, b = self._il_stage(t, w_prop, t_prop)
        wd = w.double()
        d = torch.relu(wd - b)
        term = torch.where(d > 0, d * d / (wd + (0.0 if "no_eps" in self.faults else R.EPS)), torch.zeros_like(d))
        return (term.sum() * f32c(scale)).float(), b.float()

    def interlevel_backward(self, g, w, t, w_prop, t_prop, scale):
        w, t, w_prop, t_prop = (v.float() for v in (w, t, w_prop, t_prop))
        M = w.shape[1]
        gs = self._gs(g, scale)
        e, b = self._il_stage(t, w_prop, t_prop)
        wd = w.double()
        d = wd - b
        fi = torch.where(d > 0, -2.0 * d / (wd + (0.0 if "no_eps" in self.faults else R.EPS)), torch.zeros_like(d))
        F = _excl(fi.float()).double() if "F_prefix_fp32" in self.faults else wave_prefix(fi, drop_carry="F_carry_dropped" in self.faults)
        i1 = torch.searchsorted(t[:, :M].contiguous(), e[:, 1:].contiguous(), right=False)       # count_lt(tf, M, e_j+1)
        i0 = torch.searchsorted(t[:, 1:].contiguous(), e[:, :-1].contiguous(), right=False)      # count_lt(tf + 1, M, e_j)
        out = gs * (torch.gather(F, 1, i1) - torch.gather(F, 1, i0))
        return torch.where(i1 > i0, out, torch.zeros_like(out)).float()


# ------------------------------------------------------------------------------------------------ the checks (host: Emulation; GPU: nerf_amd.ops)
def dist_case(family, N, S, mode):
    """-> (tag, (w, t), g, scale): the inputs of a case and the upstream gradient and scale it runs with"""
    fi = DIST_FAMILIES[mode].index(family)
    g, scale = pick(GS, S, fi, mode), pick(SCALES, S + 1, fi, N)
    w, t = dist_inputs(family, N, S, mode, 7000 * mode + 100 * S + 10 * fi + N % 10)
    return "distortion mode=%d %s N=%d S=%d g=%g scale=%g" % (mode, family, t.shape[0], S, g, scale), (w, t), g, scale


def il_case(family, N, M, K, open_form):
    fi = IL_FAMILIES.index(family)
    g, scale = pick(GS, M, fi, open_form), pick(SCALES, K, fi + 1, N)
    x = il_inputs(family, N, M, K, open_form, 9000 * int(open_form) + 100 * M + 10 * fi + K + N % 10)
    return "interlevel %s %s N=%d M=%d K=%d g=%g scale=%g" % ("open" if open_form else "closed", family, x[0].shape[0], M, K, g, scale), x, g, scale


def compare(tag, got, ref):
    """got {name: tensor} against ref {name: (want, tol)} -> gate items (name, value, limit): err / tol of every element under 1, and the
    exact statements (zero bounds, the NaN pattern) counted against 0"""
    items = []
    for k, v in got.items():
        items.append(("%s %s" % (tag, k), worst(v, *ref[k]), 1.0))
        items.append(("%s %s exact mismatches" % (tag, k), float(exact_mismatches(v, *ref[k])), 0.0))
    return items


def run_dist(impl, w, t, mode, g, scale):
    gt = torch.tensor(g, dtype=F32, device=w.device)
    d_w, d_t = impl.distortion_backward(gt, w, t, mode, scale)
    return {"loss": impl.distortion_loss(w, t, mode, scale), "d_w": d_w, "d_t": d_t}


def run_il(impl, x, g, scale):
    gt = torch.tensor(g, dtype=F32, device=x[0].device)
    loss, bounds = impl.interlevel_loss(*x, scale)
    return {"loss": loss, "bounds": bounds, "d_w_prop": impl.interlevel_backward(gt, *x, scale)}


# ------------------------------------------------------------------------------------------------ the old, norm-wise gates
def _old_rel(a, b):
    """test_gpu_distortion._rel on the entries where the specification is finite (generous to the old gate)"""
    a, b = a.double().cpu(), b.double().cpu()
    ok = torch.isfinite(b)
    if not bool(ok.any()):
        return 0.0
    if not bool(torch.isfinite(a[ok]).all()):
        return INF
    m = b[ok].abs().max().item()
    err = (a[ok] - b[ok]).abs().max().item()
    return err / m if m > 0 else err


def old_gate_passes(got, ref):
    """the gates of tests/test_gpu_distortion.py and tests/test_gpu_interlevel.py on the same outputs: 1e-6 relative for the loss, 1e-6 of
    the largest entry for a gradient, one ulp (2^-23) of the largest bound for bounds_out"""
    for k, v in got.items():
        lim = 2.0 ** -23 if k == "bounds" else 1e-6
        if not _old_rel(v.reshape(-1), ref[k][0].reshape(-1)) <= lim:
            return False
    return True
