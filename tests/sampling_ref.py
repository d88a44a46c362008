"""The fp64 yardstick of the sampling side (nerf_amd/csrc/sample_kernels.hip): wave_inverse_sample behind inverse_sample_kernel (both modes)
and the fused resampling kernels, and the depth draws that feed it -- stratified_points_kernel, warped_stratified_kernel, warp_depths_kernel,
length2pts_kernel.  tests/test_gpu_sampling.py compares the kernels with it element by element; tests/test_sampling_ref_host.py tests the
yardstick itself on the CPU.  The file is built with -ffp-contract=off and IEEE division: every fp32 operation below is one rounding.

SPECIFICATION.  The fp32 inputs are taken as given.

  depth draws   z = z_base[s] + u jitter                                                pts = o + d z
                s = (float)j r + u r, r = fp32(1 / C);  z = W(s) = 1 / ((1 - sb) gn + sb gf), sb = clamp(s, 0, 1)       (ray_warp_ref)
                W^-1(z) = (1 / zb - gn) / (gf - gn), zb = clamp(z, near, far);  gn = fp32(1 / near), gf = fp32(1 / far)
                length2pts = [o + d z | d]
  sample_pdf    (mode 1: bins (B), weights (B - 1); mode 0, inverse_sample: bins = the mid-points 0.5 (z[j + 1] + z[j]) in fp32, weights = w[1:-1])
                p = w + 1e-5 (fp32);  total = torch.sum(p) (fp32, ATen's cascade order);  pdf = p / total (fp32)
                cdf = [0 | torch.cumsum(pdf)]: a running sum in fp64 rounded to fp32 per element.  THIS fp32 CDF is part of the
                specification: it is the oracle's own expression (oracle.pdf_cdf), and every decision below is discrete in it.
                inds = searchsorted(cdf, u, right=True) = #{j: cdf[j] <= u}
                below = max(inds - 1, 0)     above = min(inds, nb - 1), nb = B entries
                d = fl32(cdf[above] - cdf[below]);  d < fp32(1e-5) -> D = 1, else D = cdf[above] - cdf[below]     (decision on the fp32 value)
                u >= cdf[-1] gives below == above == nb - 1, d = 0 -> D = 1, and the sample is bins[below]; u < 0 gives below == above == 0
                t = (u - cdf[below]) / D          v = bins[below] + t (bins[above] - bins[below])                  in fp64, exactly
  sort=True     the raw fp32 samples (the fp32 evaluation of the line above) in stable ascending order BY VALUE, `below` gathered by the
                same permutation (torch.sort + torch.gather, utils.py:41-43).

BOUNDS.  u = 2^-24, TINY = 2^-126, division charged 5 u as everywhere in this suite (ref_forward_ref.DIV_C), ONE = 1.01 covers products of bounds.

  stratified    m = fl(u jitter): u |m|;  z = fl(z_base + m): e(z) = u |u jitter| + u |z|
  pts           q = fl(d z^): |d| e(z) + u |d z|;  pts = fl(o + q):  e = ONE (|d| e(z) + u |d z|) + u |pts|       (e(z) = 0 where z is an input)
  coarse s      a = fl((float)j r), b = fl(u r), s = fl(a + b):  e(s) = u |j r| + u |u r| + u |s|
  W             sb: the clamp is 1-Lipschitz, e(sb) = e(s);  a = fl(1 - sb): e(a) = e(sb) + u |a|;  A = fl(a gn): ONE (e(a) gn + u |A|);
                B = fl(sb gf): ONE (e(sb) gf + u |B|);  D = fl(A + B): e(D) = e(A) + e(B) + u |D|;  z = fl(1 / D): e(z) = ONE e(D) / D^2 + 5 u |z| + TINY
  W^-1          zb exact;  r = fl(1 / zb): 5 u |r|;  n = fl(r - gn): e(n) = 5 u |r| + u |n|;  g = fl(gf - gn): u |g|;
                s = fl(n / g): e(s) = ONE (e(n) / |g| + u |s|) + 5 u |s| + TINY
  length2pts    fl(o + fl(d z)): u |d z| + u |out|;  the direction half is a copy: tolerance 0
  interpolation with the CDF and the indices fixed:
                n = fl(u - c0): u |n|;  d = fl(c1 - c0): u |d| (D = 1: exact);  t = fl(n / d): e(t) = ONE (2 u + 5 u) |t|
                w = fl(b1 - b0): u |w|;  p = fl(t w): e(p) = ONE (e(t) |w| + u |t w| + u |t w|);  v = fl(b0 + p): e(v) = e(p) + u |v|
                    e(v) = ONE 9 u |t (b1 - b0)| + u |v| + TINY
  sorted        raw_k in [v_k - e_k, v_k + e_k] for every k implies sort(raw)_i in [sort(v - e)_i, sort(v + e)_i] (order statistics are
                monotone in every element), so the sorted output is compared with the mid-point of that interval, tolerance its half width.
                `below` is discrete: the kernels' fp32 operations are IEEE and uncontracted, so their raw samples are the fp32 evaluation's,
                bit for bit, and the permutation is torch.sort's wherever neighbouring sorted values differ; inside a group of equal
                values any order is a valid sort and the multiset of `below` must agree.

WAVE SCAN.  The kernel forms the CDF with a 64-wide inclusive scan in fp64 plus a carry per chunk (device_common.h wave_incl_scan: row_shr 1,
2, 4, 8 inside rows of 16 lanes, then row_bcast:15 into rows 1 and 3, then row_bcast:31 into rows 2 and 3).  That is another ORDER of fp64
additions than cumsum's, and rounds to the same fp32 unless a running sum sits within ~2^-53 of an fp32 rounding boundary.  wave_scan_cdf
emulates it; the tests assert that it equals the oracle's CDF on every input they use, so `below`/`above` equality rests on a CPU check of
the inputs and not on the kernel's behaviour."""
import functools

import numpy as np
import torch

import ray_warp_ref as RW
from oracle import nerf_oracle as O
from ray_stages_ref import ONE, violations, worst          # noqa: F401  (one comparator for the whole per-ray family)
from ref_forward_ref import DIV_C, TINY, U

F32, F64, I64 = torch.float32, torch.float64, torch.int64
INF = float("inf")
EPS_CLAMP = float(np.float32(1e-5))
SORT_NB = 256                                              # sample_kernels.hip SORT_NB: the buckets of the sort, floor(u * 256)


def f32c(v):
    """a Python float argument as the kernel receives it"""
    return float(np.float32(v))


def ulp_step(x, up):
    return torch.nextafter(x, torch.full_like(x, INF if up else -INF))


# ------------------------------------------------------------------------------------------------ depth draws
def stratified_eval(rays, z_base, u, jitter, dt, mut=()):
    jit = f32c(jitter)
    if "jitter_wrong_count" in mut:
        jit = f32c(jitter * 0.5)                            # (far - near) / (2 S): scaled by the wrong count
    z = z_base.to(dt)[None, :] + u.to(dt) * jit
    return z, points_eval(rays, z)


def points_eval(rays, z):
    r = rays.to(z.dtype)
    return r[:, None, :3] + r[:, None, 3:] * z[:, :, None]


def _pts_tol(rays, z64, ez):
    d = rays.double()[:, None, 3:].abs()
    pts = points_eval(rays, z64)
    return ONE * (d * ez[:, :, None] + U * d * z64.abs()[:, :, None]) + U * pts.abs()


def stratified_ref(rays, z_base, u, jitter):
    """-> {"z": (want, tol), "pts": (want, tol)}"""
    z, pts = stratified_eval(rays, z_base, u, jitter, F64)
    ez = U * (u.double() * f32c(jitter)).abs() + U * z.abs()
    return {"z": (z, ez), "pts": (pts, _pts_tol(rays, z, ez))}


def warp_eval(s, near, far, mut=()):
    if "warp_no_clamp" in mut:
        gn, gf = RW.consts(near, far)
        return 1.0 / ((1.0 - s) * gn + s * gf)
    return RW.warp(s, near, far)


def _warp_tol(s64, es, near, far):
    gn, gf = RW.consts(near, far)
    sb = s64.clamp(0.0, 1.0)
    a = 1.0 - sb
    ea = es + U * a.abs()
    eA = ONE * (ea * gn + U * (a * gn).abs())
    eB = ONE * (es * gf + U * (sb * gf).abs())
    D = a * gn + sb * gf
    eD = eA + eB + U * D.abs()
    return ONE * eD / (D * D) + DIV_C * U / D.abs() + TINY


def warp_ref(s, near, far, rays=None):
    """warp_depths forward on given s -> {"out", "pts"}"""
    z = warp_eval(s.double(), near, far)
    ez = _warp_tol(s.double(), torch.zeros_like(z), near, far)
    out = {"out": (z, ez)}
    if rays is not None:
        out["pts"] = (points_eval(rays, z), _pts_tol(rays, z, ez))
    return out


def unwarp_ref(z, near, far):
    gn, gf = RW.consts(near, far)
    s = RW.unwarp(z.double(), near, far)
    zb = z.double().clamp(f32c(near), f32c(far))
    r = 1.0 / zb
    en = DIV_C * U * r.abs() + U * (r - gn).abs()
    g = abs(gf - gn)
    return {"out": (s, ONE * (en / g + U * s.abs()) + DIV_C * U * s.abs() + TINY)}


def coarse_s_eval(u, dt, mut=()):
    C = u.shape[-1]
    r = float(np.float32(1.0) / np.float32(C))
    ru = float(np.float32(1.0) / np.float32(C + 1)) if "jitter_wrong_count" in mut else r
    j = torch.arange(C, dtype=dt)
    return j * r + u.to(dt) * ru


def warped_stratified_eval(rays, u, near, far, dt, mut=()):
    s = coarse_s_eval(u, dt, mut)
    z = warp_eval(s, near, far, mut)
    return s, z, points_eval(rays, z)


def warped_stratified_ref(rays, u, near, far):
    """-> {"s", "z", "pts"}"""
    s, z, pts = warped_stratified_eval(rays, u, near, far, F64)
    C = u.shape[-1]
    r = float(np.float32(1.0) / np.float32(C))
    j = torch.arange(C, dtype=F64)
    es = U * (j * r) + U * (u.double() * r).abs() + U * s.abs()
    ez = _warp_tol(s, es, near, far)
    return {"s": (s, es), "z": (z, ez), "pts": (pts, _pts_tol(rays, z, ez))}


def length2pts_ref(rays, z):
    want = O.length2pts(rays.double(), z.double())
    tol = torch.zeros_like(want)
    d = rays.double()[:, None, 3:]
    tol[..., :3] = U * (d * z.double()[:, :, None]).abs() + U * want[..., :3].abs()
    return {"out": (want, tol)}


# ------------------------------------------------------------------------------------------------ the CDF
def _row_sum_sequential(p):
    s = torch.zeros(p.shape[0], dtype=F32)
    for j in range(p.shape[1]):
        s = s + p[:, j]
    return s[:, None]


def pdf32(weights, mut=()):
    w = weights if "no_eps" in mut else weights + 1e-5
    total = _row_sum_sequential(w) if "norm_left_to_right" in mut else torch.sum(w, -1, keepdim=True)
    return w / total


def cdf32(weights, mut=()):
    """weights (N, nw) fp32 -> the fp32 CDF (N, nw + 1) of the specification: oracle.pdf_cdf's expressions"""
    assert weights.dtype == F32
    c = torch.cumsum(pdf32(weights, mut), -1)
    c = torch.cat((torch.zeros_like(c[..., :1]), c), -1)
    if "cdf_ulp" in mut and c.shape[-1] > 2:
        c = c.clone()
        j = c.shape[-1] // 2
        c[:, j] = ulp_step(c[:, j], True)
    return c


def _wave_scan(p):
    """device_common.h wave_incl_scan on 64 doubles per row: p (N, 64) float64 -> the inclusive scan in the kernel's order of additions"""
    v = p.copy()
    for sh in (1, 2, 4, 8):                                 # row_shr:sh inside each row of 16 lanes; lanes without a source add the identity
        rows = v.reshape(-1, 4, 16)
        s = np.zeros_like(rows)
        s[:, :, sh:] = rows[:, :, :-sh]
        v = (rows + s).reshape(-1, 64)
    b = np.zeros_like(v)                                    # row_bcast:15, row mask 0xA: rows 1 and 3 add lane 15 / lane 47
    b[:, 16:32] = v[:, 15:16]
    b[:, 48:64] = v[:, 47:48]
    v = v + b
    b = np.zeros_like(v)                                    # row_bcast:31, row mask 0xC: rows 2 and 3 add lane 31
    b[:, 32:64] = v[:, 31:32]
    return v + b


def wave_scan_cdf(weights):
    """The kernel's CDF on the CPU: cascade-order normaliser, fp32 pdf, 64-wide fp64 wave scan + carry per chunk, rounded per element."""
    w = weights.numpy().astype(np.float32)
    N, nw = w.shape
    p = (w + np.float32(1e-5)).astype(np.float32)
    total = O.cascade_row_sum(p).astype(np.float32)
    pdf = (p / total[:, None]).astype(np.float32).astype(np.float64)
    cdf = np.zeros((N, nw + 1), np.float32)
    carry = np.zeros(N, np.float64)
    for base in range(0, nw, 64):
        chunk = np.zeros((N, 64), np.float64)
        n = min(64, nw - base)
        chunk[:, :n] = pdf[:, base:base + n]
        incl = _wave_scan(chunk)
        cdf[:, 1 + base:1 + base + n] = (carry[:, None] + incl[:, :n]).astype(np.float32)
        carry = carry + incl[:, 63]
    return torch.from_numpy(cdf)


def assert_wave_cdf(weights):
    """the CPU check of the inputs: the kernel's order of additions rounds to the specification's CDF"""
    assert weights.shape[-1] < 512, "cascade_row_sum covers rows of < 512 elements"
    want = cdf32(weights)
    assert torch.equal(wave_scan_cdf(weights), want), "the wave-scan order rounds differently from torch.cumsum on this input"
    return want


# ------------------------------------------------------------------------------------------------ search and interpolation
def search(cdf, u, mut=()):
    nb = cdf.shape[-1]
    inds = torch.searchsorted(cdf, u.contiguous(), right="right_false" not in mut)
    below = inds - 1 if "below_unclamped" in mut else torch.clamp(inds - 1, min=0)
    above = inds if "above_unclamped" in mut else torch.clamp(inds, max=nb - 1)
    return below, above


def _gather(row, idx):
    """row[idx] as a kernel without the clamp would read it: index -1 is the word before the row, nb the word behind it (both read as 0 here)"""
    pad = torch.cat((row, torch.zeros_like(row[..., :2])), -1)
    return torch.gather(pad, -1, torch.where(idx < 0, torch.full_like(idx, row.shape[-1] + 1), idx))


def interpolate(cdf, bins, u, below, above, dt, mut=()):
    """the sample, in dt (fp64: the specification, fp32: the emulation), and the magnitude |t (b1 - b0)| its bound needs"""
    c0, c1 = _gather(cdf, below), _gather(cdf, above)
    d32 = c1 - c0                                           # the clamp decision is taken on the fp32 value
    thr = 1e-4 if "clamp_moved" in mut else EPS_CLAMP
    clamp = torch.zeros_like(d32, dtype=torch.bool) if "clamp_absent" in mut else d32 < thr
    d = torch.where(clamp, torch.ones_like(d32, dtype=dt), c1.to(dt) - c0.to(dt))
    t = (u.to(dt) - c0.to(dt)) / d
    b0, b1 = _gather(bins, below).to(dt), _gather(bins, above).to(dt)
    tw = t * (b1 - b0)
    return b0 + tw, tw


def make_bins(z, mode, mut=()):
    if mode == 1:
        return z
    if "bins_from_depths" in mut:
        return z[..., :-1].contiguous()
    return 0.5 * (z[..., 1:] + z[..., :-1])


def make_pdf_weights(w, mode, mut=()):
    if mode == 1:
        return w
    return (w[..., :-2] if "pdf_from_0" in mut else w[..., 1:-1]).contiguous()


def sample_eval(w, z, u, mode, sort, dt=F32, mut=()):
    """fp32 (dt = F32): the emulation of inverse_sample_kernel, with planted faults `mut` -> (samples, below, above)"""
    bins, pw = make_bins(z, mode, mut), make_pdf_weights(w, mode, mut)
    cdf = cdf32(pw, mut)
    below, above = search(cdf, u, mut)
    v, _ = interpolate(cdf, bins, u, below, above, dt, mut)
    if sort:
        order = torch.sort(u if "sort_by_u" in mut else v, dim=-1, stable=True)[1]
        v = torch.gather(v, -1, order)
        if "below_unsorted" not in mut:
            below = torch.gather(below, -1, order)
    return v, below, above


def sample_ref(w, z, u, mode, sort):
    """The specification with its bounds.  sort=False -> {"v": (want, tol), "below", "above"};
    sort=True -> {"v": (want, tol), "below", "group"}: want/tol the order-statistics interval, below the value-sorted indices, group the
    id of each sorted element's run of equal fp32 values."""
    bins, pw = make_bins(z, mode), make_pdf_weights(w, mode)
    cdf = cdf32(pw)
    below, above = search(cdf, u)
    v, tw = interpolate(cdf, bins, u, below, above, F64)
    tol = ONE * 9 * U * tw.abs() + U * v.abs() + TINY
    if not sort:
        return {"v": (v, tol), "below": below, "above": above}
    raw32, _ = interpolate(cdf, bins, u, below, above, F32)
    s32, order = torch.sort(raw32, dim=-1, stable=True)
    lo, hi = torch.sort(v - tol, dim=-1)[0], torch.sort(v + tol, dim=-1)[0]
    group = torch.cumsum(torch.cat((torch.zeros_like(s32[:, :1], dtype=I64), (s32[:, 1:] != s32[:, :-1]).to(I64)), -1), -1)
    return {"v": (0.5 * (lo + hi), 0.5 * (hi - lo)), "below": torch.gather(below, -1, order), "group": group, "raw32": raw32}


def index_violations(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == I64, (got.shape, got.dtype)
    return int((got != want).sum())


def compare_unsorted(ref, v, below, above=None):
    """-> {"v": worst err / tol, "below": mismatches, "above": mismatches}"""
    out = {"v": worst(v, *ref["v"]), "below": index_violations(below, ref["below"])}
    if above is not None:
        out["above"] = index_violations(above, ref["above"])
    return out


def compare_sorted(ref, v, below=None):
    """The comparator of sorted mode -> {"descents": pairs out of order, "v": worst err / tol against the sorted specification,
    "below": mismatches -- elementwise where the specification's neighbours are distinct, as multisets inside a run of equal values}"""
    v = v.detach().cpu()
    out = {"descents": int((v[:, 1:] < v[:, :-1]).sum()) + int((~torch.isfinite(v)).sum()), "v": worst(v, *ref["v"])}
    if below is not None:
        K = v.shape[-1]
        big = int(max(int(ref["below"].max()), int(below.max()), 0)) + 2
        key = lambda b: torch.sort(ref["group"] * big + b.detach().cpu().clamp(-1, big - 2) + 1, dim=-1)[0]      # group-major, so sorting permutes only inside a group
        assert K == ref["below"].shape[-1]
        out["below"] = int((key(below) != key(ref["below"])).sum())
    return out


# ------------------------------------------------------------------------------------------------ the inputs both test modules use
NWS = (1, 3, 7, 8, 15, 32, 64, 65, 128, 129)               # + 254 (mode 0, C = 256) and 255 (mode 1, B = 256): CASES
KS = (1, 64, 65, 192, 193, 385)
W_FAMILIES = ("benign", "zero", "one_hot")
BIN_FAMILIES = ("metric", "s_space", "log", "equal_neighbours", "descending", "mixed_sign")
N_RAYS = len(W_FAMILIES) * len(BIN_FAMILIES)                # ray n: weights n % 3, bins n // 3
CASES = tuple((nw, mode) for nw in NWS for mode in (0, 1)) + ((254, 0), (255, 1))
NEAR_FAR_WARP = (0.2, 1000.0)


def _gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(repr(key).encode(), "little") % (2 ** 31 - 1))


def columns(nw, mode):
    """(columns of the weight tensor, columns of the coordinate tensor) of a case"""
    return (nw + 2, nw + 2) if mode == 0 else (nw, nw + 1)


def case_inputs(nw, mode):
    """-> (w (N, .), z (N, .)) fp32: every weight family against every bin family"""
    g = _gen("case", nw, mode)
    wc, zc = columns(nw, mode)
    w, z = torch.empty(N_RAYS, wc), torch.empty(N_RAYS, zc)
    for n in range(N_RAYS):
        wf, bf = W_FAMILIES[n % 3], BIN_FAMILIES[n // 3]
        if wf == "benign":
            w[n] = torch.rand(wc, generator=g) ** 3 + 0.01
        elif wf == "zero":
            w[n] = 0.0
        else:                                               # all the mass in one sample over a 1e-7 background: the clamp fires in every other bin
            w[n] = 1e-7
            w[n, (1 if mode == 0 else 0) + int(torch.randint(nw, (1,), generator=g))] = 1.0
        r = torch.sort(torch.rand(zc, generator=g))[0]
        if bf == "metric":
            z[n] = 2.0 + 4.0 * r
        elif bf == "s_space":
            z[n] = r ** 4
        elif bf == "log":
            z[n] = 0.2 * torch.exp(torch.linspace(0.0, float(np.log(1000.0)), zc))
        elif bf == "equal_neighbours":
            z[n] = 2.0 + torch.floor(r * max(2, zc // 3)) / max(2, zc // 3) * 4.0
        elif bf == "descending":
            z[n] = torch.flip(2.0 + 4.0 * r, (0,))
        else:
            z[n] = 6.0 * r - 3.0
    return w, z


def spec_cdf(w, z, mode):
    return cdf32(make_pdf_weights(w, mode))


ONE_BELOW_1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
U_FAMILIES = ("random", "one_bucket", "edges", "special")


def edge_uniforms(cdf, K=None):
    """every interior CDF edge, one ulp below it, itself, one ulp above it -> (N, 3 (nb - 2)) (nb = 2: one column of 0.5).
    K: exactly K columns -- an evenly spaced subset of the edges when they do not all fit, random uniforms behind them when they do."""
    e = cdf[:, 1:-1]
    if K is not None and 3 * e.shape[1] > K:
        pick = torch.linspace(0, e.shape[1] - 1, max(1, K // 3)).round().long().unique()
        e = e[:, pick]
    u = torch.cat((ulp_step(e, False), e, ulp_step(e, True)), -1)
    if K is None:
        return u if u.shape[1] else torch.full((cdf.shape[0], 1), 0.5)
    u = u[:, :K]
    fill = torch.rand(cdf.shape[0], K - u.shape[1], generator=_gen("edge fill", K, cdf.shape))
    return torch.cat((u, fill), -1).contiguous()


def uniforms(family, cdf, K, key=0):
    N = cdf.shape[0]
    g = _gen("u", family, K, key)
    if family == "random":
        return torch.rand(N, K, generator=g)
    if family == "one_bucket":                              # all of a ray's uniforms in one of the sort's 256 buckets: the rank-sort fallback
        return (77.0 + torch.rand(N, K, generator=g)) / 256.0
    if family == "edges":
        return edge_uniforms(cdf)
    sp = torch.tensor([0.0, ONE_BELOW_1, 1.0, -0.25, 1.5, float(np.float32(2.0 ** -149)), 0.5, ONE_BELOW_1, 1.0, 0.0], dtype=F32)
    u = torch.rand(N, K, generator=g)
    for n in range(N):                                      # K = 1: ray n holds special n % 10
        idx = torch.randperm(K, generator=g)[:min(K, sp.numel())]
        u[n, idx] = torch.roll(sp, n)[:idx.numel()]
    return u


def case_k(nw, mode, family):
    """the sample count of a (case, uniform family): every K of KS is met by every family across the cases"""
    i = CASES.index((nw, mode)) + U_FAMILIES.index(family)
    return KS[i % len(KS)]


def old_test_inputs(C=64, N=53, K=97):
    """the inputs of tests/test_gpu_parity.py test_inverse_sampling_indices_are_exact_for_every_row_length (its gate: below equal, max |z| error 2e-6)"""
    gen = torch.Generator().manual_seed(100 + C)
    w = torch.rand(N, C, generator=gen) ** 3 + 0.01
    z = torch.sort(2.0 + 4.0 * torch.rand(N, C, generator=gen), dim=-1)[0]
    return w, z, torch.rand(N, K, generator=gen)


# fused kernels: (C, K) -- resample_kernel's register-prefetch path, its last shape, the two generic paths
FUSED_SHAPES = ((64, 129), (128, 192), (129, 64), (64, 193))
WARPED_SHAPE = (66, 65)
N_FUSED = 9


def fused_inputs(C, K, warped=False):
    g = _gen("fused", C, K, warped)
    N = N_FUSED
    rays = torch.cat((torch.randn(N, 3, generator=g), torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1) * (0.5 + torch.rand(N, 1, generator=g))), -1)
    density = 30.0 * torch.rand(N, C, generator=g) ** 4
    density[N - 1] = 0.0                                    # an empty ray: the pdf is the blur's alpha alone
    r = torch.sort(torch.rand(N, C, generator=g), dim=-1)[0]
    if warped:
        x = r                                               # s in [0, 1]
    else:
        x = 2.0 + 4.0 * r
        x[1::3] = 0.2 * torch.exp(r[1::3] * float(np.log(1000.0)))      # log-spaced depths over [0.2, 200]
    return {"rays": rays.contiguous(), "density": density, "x": x.contiguous(), "u0": torch.rand(N, K, generator=g)}


DRAW_S = (1, 63, 64, 65)


def draw_inputs(S, N=5):
    g = _gen("draw", S)
    rays = torch.randn(N, 6, generator=g)
    u = torch.rand(N, S, generator=g)
    u[0, 0], u[N - 1, S - 1] = -0.5, 1.75                  # uniforms that leave [0, 1)
    if S > 2:
        u[1, 1], u[2, S // 2] = 1.0, 0.0
    return {"rays": rays, "u": u, "z_base": torch.linspace(2.0, 6.0, S), "jitter": 4.0 / 128,
            "z": 0.05 + 1500.0 * torch.rand(N, S, generator=g) ** 6,        # metric depths on both sides of [near, far] = [0.2, 1000]
            "s": 1.5 * torch.rand(N, S, generator=g) - 0.25}                 # s on both sides of [0, 1]


# ------------------------------------------------------------------------------------------------ the rows whose samples descend across a bucket
EXAMPLE_ROW = {
    "w": [0.022111715748906136, 0.053002454340457916, 0.26157981157302856, 0.34262925386428833, 0.025275370106101036, 0.24768735468387604],
    "z": [6.594925707759103e-07, 0.035323549062013626, 0.23793785274028778, 0.5579050779342651, 0.6729521155357361, 0.872883141040802],
    "u": [0.4609374701976776, 0.4609375], "buckets": (117, 118), "raw": [0.39792150259017944, 0.39792147278785706]}


def bucket_of(u):
    return (u * float(SORT_NB)).to(torch.int32).clamp(0, SORT_NB - 1)          # the kernel's (int)(u * 256.0f), clamped


@functools.lru_cache(maxsize=None)
def cross_bucket_rows(attempts=60000, seed=20, C=6, keep=12):
    """Rows (C = 6, inverse_sample mode 0, K = 2) whose raw fp32 samples DESCEND although the uniforms ascend, the two uniforms on the
    two sides of a bucket boundary m / 256 of the sort.  Search: bins from sorted rand(C)**4 depths; a target m / 256 that is no power of
    two; the weight in front of CDF entry j solved for cdf[j] = target and walked +-6 ulp until the fp32 CDF entry IS the target; kept
    when the sample of the uniform one ulp below the edge exceeds the sample at the edge.  EXAMPLE_ROW, the row this was first seen on, comes first.
    -> (w (R, C), z (R, C), u (R, 2), m (R,))"""
    g = torch.Generator().manual_seed(seed)
    nw = C - 2
    z = torch.sort(torch.rand(attempts, C, generator=g) ** 4, dim=-1)[0]
    w = torch.rand(attempts, C, generator=g) ** 2 + 1e-3
    m = torch.randint(3, SORT_NB, (attempts,), generator=g)
    m = torch.where((m & (m - 1)) == 0, m + 1, m)           # not a power of two
    T = (m.double() / SORT_NB)
    j = torch.randint(1, nw, (attempts,), generator=g)      # the interior CDF entry 1 .. nw - 1
    p = w[:, 1:-1].double() + 1e-5
    col = torch.arange(nw)[None, :]
    lo_mask = col < j[:, None]
    k = j - 1                                               # the solved weight: the last one in front of the edge
    pk = torch.gather(p, 1, k[:, None])[:, 0]
    A, B = (p * lo_mask).sum(1) - pk, p.sum(1) - pk
    sol = (T * B - A) / (1.0 - T)
    ok = sol > 2e-5
    w0 = w.clone()
    w0[torch.arange(attempts), k + 1] = (sol - 1e-5).clamp_min(1e-5).float()
    found_w = torch.zeros_like(w0)
    found = torch.zeros(attempts, dtype=torch.bool)
    T32 = T.float()
    for step in range(-6, 7):
        wk = w0.clone()
        x = wk[torch.arange(attempts), k + 1]
        for _ in range(abs(step)):
            x = ulp_step(x, step > 0)
        wk[torch.arange(attempts), k + 1] = x
        hit = (torch.gather(cdf32(wk[:, 1:-1].contiguous()), 1, j[:, None])[:, 0] == T32) & ok & ~found
        found_w[hit] = wk[hit]
        found |= hit
    u = torch.stack((ulp_step(T32, False), T32), -1)
    raw, _, _ = sample_eval(found_w, z, u, 0, False)
    sel = found & (raw[:, 0] > raw[:, 1])
    ex = EXAMPLE_ROW
    rows = lambda t, first: torch.cat((torch.tensor([first], dtype=t.dtype), t[sel][:keep]), 0)
    return rows(found_w, ex["w"]), rows(z, ex["z"]), rows(u, ex["u"]), rows(m, ex["buckets"][1])


# ------------------------------------------------------------------------------------------------ the planted faults of the host test
INVERSE_FAULTS = ("right_false", "no_eps", "clamp_moved", "clamp_absent", "above_unclamped", "below_unclamped", "pdf_from_0", "bins_from_depths",
                  "cdf_ulp", "norm_left_to_right", "sort_by_u", "below_unsorted")
DRAW_FAULTS = ("jitter_wrong_count", "warp_no_clamp")


# ------------------------------------------------------------------------------------------------ the checks, shared by the host and the GPU module
class Emulation:
    """The entry points the checks call, evaluated in torch fp32 on the CPU (every operation rounded on its own, like the kernels), with
    planted faults `mut`.  tests/test_gpu_sampling.py has the same interface over nerf_amd.ops."""

    def __init__(self, mut=()):
        self.mut = tuple(mut)

    def inverse(self, w, z, u, mode, sort):
        return sample_eval(w, z, u, mode, sort, F32, self.mut)

    def resample(self, inp, u, warped):
        """-> (x_fine sorted, below, w_prop, z_fine | None)"""
        x, rays = inp["x"], inp["rays"]
        zm = warp_eval(x, *NEAR_FAR_WARP) if warped else x
        w_prop = O.max_blur(O.sigma_to_weights(inp["density"], zm, rays[:, 3:]), 0.01)
        v, below, _ = sample_eval(w_prop, x, u, 0, True, F32, self.mut)
        return v, below, w_prop, (warp_eval(v, *NEAR_FAR_WARP, self.mut) if warped else None)

    def stratified(self, rays, z_base, u, jitter):
        return stratified_eval(rays, z_base, u, jitter, F32, self.mut)

    def warped_stratified(self, rays, u, near, far):
        return warped_stratified_eval(rays, u, near, far, F32, self.mut)

    def warp(self, s, near, far, rays):
        z = warp_eval(s, near, far, self.mut)
        return z, points_eval(rays, z)

    def unwarp(self, z, near, far):
        return RW.unwarp(z, near, far)

    def length2pts(self, rays, z):
        return O.length2pts(rays, z)


def _inverse_gates(impl, tag, w, z, u, mode, sorts):
    out = []
    for sort in sorts:
        ref = sample_ref(w, z, u, mode, sort)
        v, below, above = impl.inverse(w, z, u, mode, sort)
        res = compare_sorted(ref, v, below) if sort else compare_unsorted(ref, v, below, above)
        for k, x in res.items():
            out.append(("sampling %s sort=%d %s" % (tag, sort, k), x, 1.0 if k == "v" else 0))
    return out


def inverse_case_gates(impl, nw, mode):
    """one (row length, mode): every weight family x bin family (the rays) against every uniform family -> [(name, value, limit)].
    mode 0 is ops.inverse_sample (both sort values, no `above`), mode 1 ops.sample_pdf (unsorted, with `above`)."""
    w, z = case_inputs(nw, mode)
    cdf = assert_wave_cdf(make_pdf_weights(w, mode))
    out = []
    for fam in U_FAMILIES:
        u = uniforms(fam, cdf, case_k(nw, mode, fam))
        out += _inverse_gates(impl, "nw=%d mode=%d K=%d u=%s" % (nw, mode, u.shape[1], fam), w, z, u, mode, (False, True) if mode == 0 else (False,))
    return out


def sample_count_gates(impl, K):
    """every K of KS at one row length on both sides of the 192-sample search chunk, all four uniform families (edges: padded or cut to K)"""
    nw, mode = 64, 0
    w, z = case_inputs(nw, mode)
    cdf = assert_wave_cdf(make_pdf_weights(w, mode))
    out = []
    for fam in U_FAMILIES:
        u = edge_uniforms(cdf, K) if fam == "edges" else uniforms(fam, cdf, K, key=1)
        out += _inverse_gates(impl, "nw=%d mode=%d K=%d u=%s (K sweep)" % (nw, mode, K, fam), w, z, u, mode, (False, True))
    return out


def cross_bucket_gates(impl):
    w, z, u, _ = cross_bucket_rows()
    assert_wave_cdf(make_pdf_weights(w, 0))
    out = _inverse_gates(impl, "cross-bucket rows K=2", w, z, u, 0, (False, True))
    pad = torch.rand(w.shape[0], 63, generator=_gen("cross pad"))
    return out + _inverse_gates(impl, "cross-bucket rows K=65", w, z, torch.cat((pad[:, :30], u, pad[:, 30:]), -1).contiguous(), 0, (False, True))


def fused_gates(impl, C, K, warped):
    """ops.resample / ops.warped_resample in two calls: the first returns the device's own w_prop, the edge uniforms of ITS CDF go into the second"""
    inp = fused_inputs(C, K, warped)
    _, _, w_prop, _ = impl.resample(inp, inp["u0"], warped)
    w_prop = w_prop.detach().cpu()
    cdf = assert_wave_cdf(w_prop[:, 1:-1].contiguous())
    u = edge_uniforms(cdf, K)
    v, below, w2, zf = impl.resample(inp, u, warped)
    tag = "sampling fused %s C=%d K=%d " % ("warped_resample" if warped else "resample", C, K)
    out = [(tag + "w_prop differs between the two calls", violations(w2.detach().cpu(), w_prop), 0)]
    ref = sample_ref(w_prop, inp["x"], u, 0, True)
    for k, x in compare_sorted(ref, v, below).items():
        out.append((tag + k, x, 1.0 if k == "v" else 0))
    if warped:
        out.append((tag + "z_fine = W(s_fine)", worst(zf, *warp_ref(v.detach().cpu(), *NEAR_FAR_WARP)["out"]), 1.0))
    return out


def _named(tag, ref, got):
    return [("sampling %s %s" % (tag, k), worst(got[k], *ref[k]), 1.0) for k in ref]


def draw_gates(impl, S):
    d = draw_inputs(S)
    rays, u = d["rays"], d["u"]
    out = []
    z, pts = impl.stratified(rays, d["z_base"], u, d["jitter"])
    out += _named("stratified_points S=%d" % S, stratified_ref(rays, d["z_base"], u, d["jitter"]), {"z": z, "pts": pts})
    out += _named("length2pts S=%d" % S, length2pts_ref(rays, d["z"]), {"out": impl.length2pts(rays, d["z"])})
    for near, far in ((2.0, 6.0), NEAR_FAR_WARP):
        tag = "S=%d near=%g far=%g" % (S, near, far)
        zz, pts = impl.warp(d["s"], near, far, rays)
        out += _named("warp_depths " + tag, warp_ref(d["s"], near, far, rays), {"out": zz, "pts": pts})
        out += _named("warp_depths inverse " + tag, unwarp_ref(d["z"], near, far), {"out": impl.unwarp(d["z"], near, far)})
        if S >= 3:                                          # (nerf_amd_warped_stratified takes 3 <= C <= 256)
            s, zz, pts = impl.warped_stratified(rays, u, near, far)
            out += _named("warped_stratified " + tag, warped_stratified_ref(rays, u, near, far), {"s": s, "z": zz, "pts": pts})
    return out


DRAW_SIZES = DRAW_S + (3,)                                  # 3: the shortest row warped_stratified takes
