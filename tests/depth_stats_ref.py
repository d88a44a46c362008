"""Quantile ray-termination depths and accumulated opacity (nerf_amd_ray_depth_stats, include/nerf_amd.h) for the tests: the fp64
specification, a brute-force restatement ray by ray, the per-element error bound of an fp32 implementation with its derivation, the checker
built on the two, and the input generator.  numpy only; nothing of the package is imported.

Specification.  Per ray: weights w_0 .. w_{S-1} (fp32, >= 0), depths z_0 .. z_{E-1} with E = S + 1 (closed: the row also holds the edge
that closes the last interval) or E = S (open), direction d; t_s = z_s |d| with mul_norm, else t_s = z_s.
    C_0 = 0, C_{s+1} = C_s + (double)w_s                      cumulative mass in fp64, ABSOLUTE (not renormalised)
    opacity = (float)C_S
    for a quantile q (an fp32 value, 0 < q < 1):  k = the smallest s with C_{s+1} >= q
        no such s (the ray never accumulates q)     D_q = t_{E-1}
        k = S - 1 and the row is open               D_q = t_{S-1}
        otherwise                                   D_q = t_k + ((q - C_k) / w_k) (t_{k+1} - t_k)     fp64, rounded once to fp32
    output (D_q - near) / (far - near)
The specification evaluates all of it in fp64 (|d| and t included) on the fp32 inputs.

Error bound of the HIP kernel against the specification, per (ray, q); u = 2^-24 (half an fp32 ulp, relative):
  (a) t.  The kernel forms |d| = sqrt((x x + y y) + z z) and t = z |d| in fp32.  Three products and two sums of positive terms, each rounded
      (or fewer roundings where a compiler contracts a product into an FMA: never more): the sum of squares is within 3u, its root within
      1.5u + u = 2.5u, the product z |d| within 3.5u: |t^ - t| <= 4u |t| (first order; the factor (1 + 2^-20) below covers the rest).
      Without mul_norm t^ = z exactly.  D_q is a convex combination of t_k and t_{k+1} ((q - C_k) / w_k lies in [0, 1]), so it inherits at
      most max(e_t(k), e_t(k+1)); in the two fall-back cases it IS one t.
  (b) C.  Any fp64 summation order of S non-negative terms is within (S - 1) 2^-53 C_S of the exact sum: the kernel's wave scan and the
      specification's own sequential sum differ by delta <= 2 S 2^-53 C_S in every prefix.  D_q = F^-1(q) for the piecewise-linear F through
      (t_s, C_s); moving every knot's C by at most delta moves F^-1(q) by at most delta times the steepest slope (t_{j+1} - t_j) / w_j of
      an interval with w_j > 0 whose mass range [C_j, C_{j+1}] meets [q - WINDOW, q + WINDOW] (WINDOW = 1e-12 >= delta, asserted).  Where
      that window also holds an edge next to a ZERO-weight interval F^-1 jumps and no bound exists: those pairs are reported as excluded
      (the only exclusion; D_q is continuous everywhere else, the two fall-back cases included: a closed row's t_S is the limit of the
      last interval's interpolation, an open row returns t_{S-1} from both sides).
  (c) the interpolation itself in fp64: a few 2^-53 |t|, covered by 16 * 2^-53 * max|t| of the row.
  (d) the one rounding of D_q to fp32: u |D_q|.
  (e) the normalisation in fp32, fl(fl(D - near) / fl(far - near)): three roundings, 3u |D - near| / |far - near|, on top of the error
      of D divided by |far - near|.
    tol = ((a) + (b) + (c) + (d)) / |far - near| + (e)
Opacity: the kernel's C_S and the specification's agree to delta (1e-13 relative), so their fp32 roundings are equal or neighbours: 1 ulp.
"""
import numpy as np

U = 2.0 ** -24
WINDOW = 1e-12
QUANTILES_MAX = 4


def _evaluate(w, z, dirs, quantiles, near, far, mul_norm, cum_dtype=np.float64, renormalise=False, edge_shift=0, use_norm=True):
    """The specification; the last four arguments exist only so that tests can plant faults (fp32 cumsum, renormalised mass, off-by-one
    edge, a forgotten |d|).  -> dict: depth_q (N,Q) fp64, opacity (N,) fp64, D (N,Q), k (N,Q; -1: never reached), C (N,S+1), t (N,E)"""
    w = np.asarray(w, dtype=np.float32)
    z = np.asarray(z, dtype=np.float32)
    N, S = w.shape
    E = z.shape[1]
    assert E in (S, S + 1) and S >= 1
    q32 = np.asarray(quantiles, dtype=np.float32).reshape(-1)
    assert q32.size <= QUANTILES_MAX and np.all((q32 > 0) & (q32 < 1))
    nrm = np.ones(N)
    if mul_norm and use_norm:
        d = np.asarray(dirs, dtype=np.float32).astype(np.float64)[:, -3:]
        nrm = np.sqrt((d * d).sum(1))
    t = z.astype(np.float64) * nrm[:, None]
    C = np.concatenate((np.zeros((N, 1), cum_dtype), np.cumsum(w.astype(cum_dtype), axis=1, dtype=cum_dtype)), 1).astype(np.float64)
    w64 = w.astype(np.float64)
    if renormalise:
        total = np.maximum(C[:, -1:], 1e-300)
        C, w64 = C / total, w64 / total
    rows = np.arange(N)
    D = np.empty((N, q32.size))
    K = np.empty((N, q32.size), dtype=np.int64)
    for j, q in enumerate(q32.astype(np.float64)):
        reach = C[:, 1:] >= q
        hit = reach.any(1)
        k = np.where(hit, reach.argmax(1), S - 1)
        lo = np.minimum(k + edge_shift, E - 1)
        hi = np.minimum(k + 1 + edge_shift, E - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = (q - C[rows, k]) / w64[rows, k]                       # (rows that never reach q: discarded below)
            interp = t[rows, lo] + f * (t[rows, hi] - t[rows, lo])
        D[:, j] = np.where(hit, np.where(k + 1 < E, interp, t[rows, lo]), t[:, E - 1])
        K[:, j] = np.where(hit, k, -1)
    nf, ff = np.float64(np.float32(near)), np.float64(np.float32(far))
    return {"depth_q": (D - nf) / (ff - nf), "opacity": C[:, -1].copy(), "D": D, "k": K, "C": C, "t": t, "q": q32.astype(np.float64)}


def spec(w, z, dirs=None, quantiles=(0.5,), near=0.0, far=1.0, mul_norm=True):
    return _evaluate(w, z, dirs, quantiles, near, far, mul_norm and dirs is not None)


def brute(w, z, dirs=None, quantiles=(0.5,), near=0.0, far=1.0, mul_norm=True):
    """The definition read aloud, one ray and one quantile at a time in Python floats (= fp64).  -> (depth_q (N,Q), opacity (N,))"""
    w = np.asarray(w, dtype=np.float32)
    z = np.asarray(z, dtype=np.float32)
    N, S = w.shape
    E = z.shape[1]
    qs = [float(np.float32(q)) for q in quantiles]
    near, far = float(np.float32(near)), float(np.float32(far))
    out, opacity = np.empty((N, len(qs))), np.empty(N)
    for n in range(N):
        nrm = 1.0
        if mul_norm and dirs is not None:
            d = [float(v) for v in np.asarray(dirs, dtype=np.float32)[n, -3:]]
            nrm = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) ** 0.5
        t = [float(v) * nrm for v in z[n]]
        for j, q in enumerate(qs):
            c, depth = 0.0, t[E - 1]                              # the ray never accumulates q: the far edge
            for s in range(S):
                c_next = c + float(w[n, s])
                if c_next >= q:
                    depth = t[s] if s + 1 >= E else t[s] + (q - c) / float(w[n, s]) * (t[s + 1] - t[s])
                    break
                c = c_next
            out[n, j] = (depth - near) / (far - near)
        c = 0.0
        for s in range(S):
            c += float(w[n, s])
        opacity[n] = c
    return out, opacity


def tolerance(ref, w, near, far, mul_norm):
    """-> (tol (N,Q) on depth_q, excluded (N,Q) bool) for the specification's result `ref` (see the module docstring)"""
    w64 = np.asarray(w, dtype=np.float32).astype(np.float64)
    C, t, D, K = ref["C"], ref["t"], ref["D"], ref["k"]
    N, S = w64.shape
    E = t.shape[1]
    rows = np.arange(N)
    e_t = (4.0 * U * (1.0 + 2.0 ** -20)) * np.abs(t) if mul_norm else np.zeros_like(t)
    delta = 2.0 * S * 2.0 ** -53 * C[:, -1]
    assert np.all(delta <= WINDOW), "the window of (b) must cover the accumulation error"
    t_next = t[:, 1:] if E == S + 1 else np.concatenate((t[:, 1:], t[:, -1:]), 1)              # (N,S): open rows have no edge behind the last interval
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(w64 > 0, (t_next - t[:, :S]) / w64, 0.0)
    zero_left = np.concatenate((np.zeros((N, 1), bool), w64 == 0), 1)                          # (N,S+1): the interval below edge s is empty
    zero_right = np.concatenate((w64 == 0, np.zeros((N, 1), bool)), 1)
    B = abs(float(np.float32(far)) - float(np.float32(near)))
    tol = np.empty_like(D)
    excluded = np.zeros(D.shape, bool)
    for j, q in enumerate(ref["q"]):
        k = K[:, j]
        kk = np.where(k >= 0, k, E - 1)
        interp = (k >= 0) & (k + 1 < E)
        a = np.where(interp, np.maximum(e_t[rows, np.minimum(kk, E - 1)], e_t[rows, np.minimum(kk + 1, E - 1)]), e_t[rows, np.minimum(kk, E - 1)])
        near_q = (C[:, :-1] <= q + WINDOW) & (C[:, 1:] >= q - WINDOW) & (w64 > 0)
        b = delta * np.where(near_q, slope, 0.0).max(1)
        c = 16.0 * 2.0 ** -53 * np.abs(t).max(1)
        d = U * np.abs(D[:, j])
        e = 3.0 * U * (1.0 + 2.0 ** -20) * np.abs(D[:, j] - float(np.float32(near))) / B
        tol[:, j] = (a + b + c + d) / B + e
        excluded[:, j] = ((np.abs(C - q) < WINDOW) & (zero_left | zero_right)).any(1)
    return tol, excluded


def check(depth_q, opacity, w, z, dirs=None, quantiles=(0.5,), near=0.0, far=1.0, mul_norm=True):
    """An implementation's fp32 results against the specification.  -> (worst err / tol over the pairs that count -- <= 1 passes --,
    worst opacity error in fp32 ulps of the specification's value, number of excluded pairs, number of pairs)"""
    mul = bool(mul_norm and dirs is not None)
    ref = spec(w, z, dirs, quantiles, near, far, mul)
    tol, excluded = tolerance(ref, w, near, far, mul)
    ratio = 0.0
    if depth_q is not None and ref["q"].size:
        got = np.asarray(depth_q, dtype=np.float64).reshape(ref["depth_q"].shape)
        err = np.where(excluded, 0.0, np.abs(got - ref["depth_q"]) / tol)
        err = np.where(np.isfinite(got) | excluded, err, np.inf)
        ratio = float(err.max()) if err.size else 0.0
    ulps = 0.0
    if opacity is not None:
        want = ref["opacity"].astype(np.float32)
        spacing = np.maximum(np.spacing(np.abs(want)), np.float32(2.0 ** -149)).astype(np.float64)
        got = np.asarray(opacity, dtype=np.float64).reshape(-1)
        ulps = float((np.abs(got - want.astype(np.float64)) / spacing).max()) if want.size else 0.0
    return ratio, ulps, int(excluded.sum()), int(excluded.size)


# S of the device sweep: one lane, two, one short of a chunk, a chunk, one past it, two chunks, one past them, a ragged row, the Ref-NeRF maximum
GPU_S = (1, 2, 63, 64, 65, 128, 129, 300, 1087)
GPU_N = (1, 3, 5, 67)


def make_inputs(N, S, closed, seed):
    """fp32 (w (N,S), z (N,E), dirs (N,3)).  Depths sorted 2 + 4 rand, directions of norm 0.5 .. 2.5.  Ray n is of kind (n + seed) % 5:
      0  dense: rand weights, total mass 0.6 .. 1
      1  the same with about a third of the weights exactly zero
      2  one spike of 0.875 in an otherwise empty row, at sample 63, 64, S - 1 or 0 by turns: q below it interpolates inside the spike,
         q above it is never reached
      3  dense, total mass 0.3: every q >= 0.3 reports the far edge
      4  a background of total mass 0.2 and one weight of 0.6 at sample 63 (even n) or 64 (odd n): q = 0.5 crosses in the last lane of a
         chunk or in lane 0 of the next one (rows shorter than that: at S - 1)
    Spikes and totals are dyadic or far from every q the tests use, so no crossing sits on an edge next to an empty interval."""
    g = np.random.default_rng(1000003 * seed + 1009 * S + N)
    E = S + (1 if closed else 0)
    z = np.sort(2.0 + 4.0 * g.random((N, E)), axis=1).astype(np.float32)
    dirs = g.standard_normal((N, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * (0.5 + 2.0 * g.random((N, 1)))).astype(np.float32)
    w = np.zeros((N, S))
    for n in range(N):
        kind = (n + seed) % 5
        r = g.random(S) + 1e-3
        if kind == 0:
            w[n] = r / r.sum() * (0.6 + 0.4 * g.random())
        elif kind == 1:
            r = r * (g.random(S) > 0.33)
            if r.sum() == 0.0:
                r[0] = 1.0
            w[n] = r / r.sum() * (0.6 + 0.4 * g.random())
        elif kind == 2:
            w[n, min((63, 64, S - 1, 0)[(n // 5) % 4], S - 1)] = 0.875
        elif kind == 3:
            w[n] = r / r.sum() * 0.3
        else:
            at = min(63 + (n & 1), S - 1)
            r[at] = 0.0
            w[n] = r / max(r.sum(), 1e-30) * 0.2 if S > 1 else 0.0
            w[n, at] = 0.6
    return w.astype(np.float32), z, dirs
