"""The fp64 specification of the input encoding of the proposal and fine kernels -- everything between the sample descriptor and the first
MFMA -- and the derivation of every per-element bound the GPU tests hold the kernels to.  Plain helper module (no fixtures), in the manner
of ipe_gaussian_ref.py and ray_stages_ref.py; the error calculus (`Fl`, `fma`, `fl_sin`, `fl_cos`, `fl_exp`), the frustum moments
(`fl_moments`, `cone_moments`) and the integrated-PE bounds (`kernel_bounds`, modes "plain" and "metric") are ipe_gaussian_ref's, imported,
not copied.  tests/test_encoding_ref_host.py checks this module on the CPU (against the oracle and the goldens, an fp32 emulation inside
every bound, fourteen planted faults outside them); tests/test_gpu_encoding.py feeds it what the kernels wrote.

Every function takes the kernel's own fp32 inputs and returns an `Fl`: the fp64 value v of every output element and a bound e on
|computed - v| for every element, obtained by propagating the operations IN THE ORDER THE CODE PERFORMS THEM (u = 2^-24; the rules for
+, *, /, sqrt, fma, exp and the 2^-126 each operation pays for a flushed or denormal result are in ipe_gaussian_ref's docstring).  The
build uses -ffp-contract=off, so a product and a sum round separately unless the code says fma.  The sequences:

SAMPLE POSITION (mlp_kernels.hip fetch_sample; `positions`)
  mode 0   x = pts[m stride + 0..2], d = pts[m stride + 3..5]: inputs, exact.
  mode 1   ray n = m / S, sample s = m - n S;  o = rays[6 n + 0..2], d = rays[6 n + 3..5]: exact.
           depth:  z = z[n z_stride + s] (exact), or  z = z_base[s] + fl(u[n S + s] z_jitter)   (a product, then a sum)
           x_c = o_c + fl(z d_c)                                                               (a product, then a sum)
  mode 2   row = n / W, col = n - row W;  cx = ((col - W/2) + 1/2) / fx,  cy = ((H/2 - row) + 1/2) / fy   (the differences and the halves
           are exact for image sizes below 2^23; they are propagated as roundings all the same, which only loosens the bound by 2 u);
           d_c = (fl(cx P[c][0]) + fl(cy P[c][1])) + (-P[c][2]),  o_c = P[c][3];  depth and position as in mode 1.
CONTRACTION (contract_position; `contract`)
  n = sqrt((x x + y y) + z z);  if n > 1:  k = (2 - 1 / n) / n,  x_c <- fl(x_c k)     (three products, two divisions, one root)
  The branch is taken on the fp32 norm, whose bound is a few u: the test inputs keep every position (and every metric frustum mean)
  further than SPHERE_GAP = 1e-4 from the unit sphere, `contract` returns the smallest distance and the tests assert it for ALL
  samples (excluded share 0).
DIRECTION (`normalise`)   n = sqrt((dx dx + dy dy) + dz dz);  dh_c = d_c / n (three divisions);  then the PE with L = 4.
POSITIONAL ENCODING (`pe`; columns in the reference's order: per octave l the three sines, then the three cosines)
  path "direct"    the fp32 fused kernels, pe_kernel: a_l = 2^l x (exact), sin_quadrant(a_l, 0 | 1): e = 2^l e_x + sincos_abs(a_l)
                   (ipe_gaussian_ref SIN_QUADRANT: 4 u up to |a| = 2^21, refused beyond).  Ten separate range reductions at L = 10.
  path "doubling"  the bf16 fused kernels (encode, encode_pair) and the direction table: octave 0 as above, then per octave
                   s' = fl(fl(2 s) c), c' = fma(-2 s, s, 1).  The exact values obey the same identities; the errors follow
                   e_s' = 2 (|s| e_c + |c| e_s + e_s e_c) + u |s'|,  e_c' = 4 |s| e_s + 2 e_s^2 + u |c'|: they can quadruple per octave, so the
                   worst case at octave 9 is 4^9 . 4 u = 0.06.  The comment in mlp_kernels.hip says 2^9 . 1e-7 = 5e-5; that follows an
                   angle error alone.  The recurrence also takes (s, c) off the unit circle, and a radial error eps becomes
                   4 eps sin^2(theta): a factor 3 per step on the orbit 2 pi / 3 <-> 4 pi / 3.  The fp32 emulation reaches 2e4 u =
                   1.3e-3 at octave 9 (test_encoding_ref_host.py) -- below the bf16 half-ulp of a feature of size 1/2 .. 1, above
                   that of a small one.  DESIGN.md section 4 records it; the bound here is the propagated one, not the comment's.
  path "libm"      encode_rows_kernel calls the device library's sincosf, not sin_quadrant: generic_ref.py's allowance for a device math
                   function, FN_U u = 4 u (its docstring: documented at 1 ulp, 1 ulp <= 2 u, doubled because it comes from testing).
                   "libm-doubling": its bf16 rows take octave 0 from sincosf and double from there.
INTEGRATED PE   ipe_gaussian_ref.kernel_bounds with mode "plain" (contract = 0) or "metric" (contract = 1: the mean through the
                contraction, the covariance left alone): fl_moments, cone_mean_cov, [contract], then per level either its own reduction
                and its own expf ("direct") or the doubling recurrences with att <- (att^2)^2 ("doubling").
STORED BF16 (`bf16_stored`)   anything read from a bf16 dump, row or table: Fl.stored_bf16 (+ 2^-8 (|v| + e)) + 2^-126: an fp32 denormal
                becomes a bf16 denormal (spacing 2^-133) or is flushed (|v| < 2^-126), either way within 2^-126.
RAW SLOTS       x, y | z, 0 (or mu): the position's own bound; where the position is an input (mode 0, no contraction) the fp32 slot must
                hold its bits.  In bf16 only the conversion is added.
PADDING         exactly 0 (e = 0: any other value counts as inf).

THE COMPARATOR (`compare`): {output: max(err / tol)}, a non-finite value or an error where e = 0 counts as inf.

FITTED CONSTANTS: none.  Every allowance is a property of the number formats, of the sequence of operations, or of the literals in
device_common.h (SIN_QUADRANT), or is generic_ref's documented allowance for a device math function.

THE INPUTS (`ray_batch`, `depth_rows`, `point_batch`, `clear_of_sphere`): shared by the host test and the GPU test, so that the fp32
emulation is shown inside every bound on exactly the inputs the kernels get.  Every batch mixes its families by n % k:
  magnitudes of the workload (near 2, far 6, origins in [-0.5, 0.5]^3); coordinates 0, -0 and denormals; positions just inside and just
  outside |x| = 1 (2e-4 .. 2e-2 away); |x| up to far |d| at far = 1000 (contraction off: the largest octave-9 argument is 1.54e6); thin
  frusta (hw / mid = 1e-4), degenerate ones (z0 == z1); ipe_gaussian_ref's geometric family out to 1e6 (contraction on only: without it
  2^9 . 1e6 is outside SINCOS_DOMAIN -- a domain the header now states); un-normalised directions with |d| in [0.3, 3]."""
import math

import torch

import generic_ref as GR
import ipe_gaussian_ref as G
from ipe_gaussian_ref import Fl, fma, fl_sin, fl_cos, fl_exp, fl_moments, cone_moments, make_inputs, sphere_gap  # noqa: F401  (re-exported)
from ipe_gaussian_ref import SPHERE_GAP, TINY, U

LIBM_SINCOS = GR.FN_U * U                       # sincosf of the device library: generic_ref's 2 ulp = 4 u
NEAR, FAR, FAR_WIDE = 2.0, 6.0, 1000.0
DN_FLOOR = 16.0                                 # the IPE tests hand the kernels dn = max(|D|, 16): > max d_c^2 = 9, so 1 - d_c^2 / dn > 0


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def col(a, c):
    return Fl(a.v[..., c: c + 1], a.e[..., c: c + 1])


def cat(parts, dim=-1):
    shape = torch.broadcast_shapes(*[p.v.shape[:-1] for p in parts]) if dim == -1 else None
    if shape is not None:
        parts = [Fl(p.v.expand(shape + p.v.shape[-1:]), p.e.expand(shape + p.e.shape[-1:])) for p in parts]
    return Fl(torch.cat([p.v for p in parts], dim), torch.cat([p.e for p in parts], dim))


def bf16_stored(a):
    b = a.stored_bf16()
    return Fl(b.v, b.e + TINY)


def norm3(a):
    x, y, z = col(a, 0), col(a, 1), col(a, 2)
    return ((x * x + y * y) + z * z).sqrt()


# ------------------------------------------------------------------------------------------------ sample position
def positions(src):
    """src: a dict describing a sample descriptor (CPU fp32 tensors / Python numbers):
         {"mode": 0, "pts": (M, stride)}
         {"mode": 1, "rays": (N, 6), "S": S, "z": (N, z_stride >= S)}   or   ... "z_base": (S,), "u": (N, S), "z_jitter": float
         {"mode": 2, "pose": 12 floats, "H", "W", "fx", "fy", "N": rays, "S", and the depths as in mode 1}
    -> (x (M, 3), d (M, 3) or None when the source has no direction columns): Fl, in fetch_sample's order of operations."""
    if src["mode"] == 0:
        p = src["pts"].double()
        return Fl(p[:, :3].clone()), (Fl(p[:, 3:6].clone()) if p.shape[1] >= 6 else None)
    S = src["S"]
    if src["mode"] == 1:
        r = src["rays"].double()
        o, d = Fl(r[:, None, :3]), Fl(r[:, None, 3:6])
        N = r.shape[0]
    else:
        N, W, H = src["N"], src["W"], src["H"]
        P = [float(v) for v in src["pose"]]
        n = torch.arange(N, dtype=torch.float64)
        row = torch.div(n, W, rounding_mode="floor")
        cl = n - row * W
        cx = ((Fl(cl) - Fl(W * 0.5)) + Fl(0.5)) / Fl(f32(src["fx"]))
        cy = ((Fl(H * 0.5) - Fl(row)) + Fl(0.5)) / Fl(f32(src["fy"]))
        comps = [(cx * Fl(P[4 * c]) + cy * Fl(P[4 * c + 1])) + Fl(-P[4 * c + 2]) for c in range(3)]
        d = Fl(torch.stack([c.v for c in comps], -1)[:, None, :], torch.stack([c.e for c in comps], -1)[:, None, :])
        o = Fl(torch.tensor([P[3], P[7], P[11]], dtype=torch.float64)[None, None, :])
    if src.get("z") is not None:
        z = Fl(src["z"][:, :S].double()[..., None])
    else:
        z = Fl(src["z_base"].double()[None, :, None]) + Fl(src["u"].double()[..., None]) * Fl(f32(src["z_jitter"]))
    x = o + z * d
    M = N * S
    return Fl(x.v.reshape(M, 3), x.e.reshape(M, 3)), Fl(d.v.expand(N, S, 3).reshape(M, 3), d.e.expand(N, S, 3).reshape(M, 3))


def contract(x):
    """-> (the contracted position, min | |x| - 1 | over the exact norms)"""
    n = norm3(x)
    outside = n.v > 1
    gap = float((n.v - 1).abs().min()) if n.v.numel() else float("inf")
    ns = n.where(outside, Fl(torch.full_like(n.v, 2.0)))
    k = (Fl(2.0) - Fl(1.0) / ns) / ns
    return (x * k).where(outside.expand_as(x.v), x), gap


def normalise(d):
    return d / norm3(d)


# ------------------------------------------------------------------------------------------------ positional encoding
def _libm(a, fn):
    return Fl(fn(a.v), a.e + LIBM_SINCOS)


def pe(x, L, path):
    """x Fl (..., 3) -> Fl (..., 6 L) in the reference's column order"""
    first = (lambda a: (fl_sin(a), fl_cos(a))) if path in ("direct", "doubling") else (lambda a: (_libm(a, torch.sin), _libm(a, torch.cos)))
    out = []
    if path in ("direct", "libm"):
        for l in range(L):
            out += list(first(x.scaled(2.0 ** l)))
    else:
        s, c = first(x)
        for l in range(L):
            out += [s, c]
            s2 = s.scaled(2.0)
            s, c = s2 * c, fma(s2.scaled(-1.0), s, Fl(1.0))
    return cat(out)


def encode_rows(x, L, normalize, bf16):
    """nerf_amd_encode_rows: [x | PE_L(x) | 0 pad] -> {"raw": (M, 3), "pe": (M, 6 L), "pad": zeros}"""
    x = Fl(x.double()[:, :3].clone())
    if normalize:
        x = normalise(x)
    feat = pe(x, L, "libm-doubling" if bf16 else "libm")
    ncol = (3 + 6 * L + 7) // 8 * 8
    pad = Fl(torch.zeros(x.v.shape[0], ncol - 3 - 6 * L, dtype=torch.float64))
    if bf16:
        x, feat = bf16_stored(x), bf16_stored(feat)
    return {"raw": x, "pe": feat, "pad": pad}


def ipe(z, rays, L, r2, dn, mode, path="direct", bf16=False):
    """the integrated PE of the frusta between consecutive depths: z (N, S + 1) -> {"pe": (M, 6 L), "raw": mu (M, 3)}, metric gap"""
    b = G.kernel_bounds(z, rays, L, r2, dn, mode=mode, path=path)
    M = b["mu"].v.shape[0] * b["mu"].v.shape[1]
    feat, mu = Fl(b["feat"].v.reshape(M, 6 * L), b["feat"].e.reshape(M, 6 * L)), Fl(b["mu"].v.reshape(M, 3), b["mu"].e.reshape(M, 3))
    if bf16:
        feat, mu = bf16_stored(feat), bf16_stored(mu)
    return {"pe": feat, "raw": mu}


def fused(src, net, prec, contracted, ipe_args=None):
    """The encoding slot of proposal_forward_train / mip_forward_train on descriptor `src`, in the reference's column order:
    {"pos-raw": (M, 3), "pos-pe": (M, 60)[, "dir-raw": (M, 3), "dir-pe": (M, 24)]} and the sphere gap (inf without contraction).
    ipe_args = (r2, dn): the integrated PE (mode 1 with explicit z of S + 1 depths)."""
    bf16 = prec == "bf16"
    path = "doubling" if bf16 else "direct"
    x, d = positions(src)
    gap = float("inf")
    if ipe_args is not None:
        z = src["z"][:, : src["S"] + 1].contiguous()
        out = ipe(z, src["rays"], 10, ipe_args[0], ipe_args[1], "metric" if contracted else "plain", path, bf16)
        out = {"pos-raw": out["raw"], "pos-pe": out["pe"]}
        if contracted:
            gap = sphere_gap(z, src["rays"])
    else:
        if contracted:
            x, gap = contract(x)
        feat = pe(x, 10, path)
        out = {"pos-raw": bf16_stored(x) if bf16 else x, "pos-pe": bf16_stored(feat) if bf16 else feat}
    if net == "mip":
        dh = normalise(d)
        feat = pe(dh, 4, path)
        out["dir-raw"], out["dir-pe"] = (bf16_stored(dh), bf16_stored(feat)) if bf16 else (dh, feat)
    return out, gap


def direction_table(rays):
    """nerf_amd_direction_table: {"dir-raw", "dir-pe"} of every ray (the bf16 doubling path, stored as bf16)"""
    dh = normalise(Fl(rays[:, 3:6].double().clone()))
    return {"dir-raw": bf16_stored(dh), "dir-pe": bf16_stored(pe(dh, 4, "doubling"))}


def cone_parameters(z, r2):
    mu_t, var_t, var_r = fl_moments(z, r2)
    sq = lambda a: Fl(a.v[..., 0], a.e[..., 0])
    return {"mu_t": sq(mu_t), "var_t": sq(var_t), "var_r": sq(var_r)}


def dirs_norm(rays):
    """one workgroup, fp64 partial sums in a fixed order, (float) sqrt: the fp64 value rounded once, plus the fp64 accumulation's
    N 2^-52 relative"""
    v = (rays[:, 3:6].double() ** 2).sum().sqrt().reshape(1)
    return {"dn": Fl(v, v * (U + rays.shape[0] * 2.0 ** -52) + TINY)}


# ------------------------------------------------------------------------------------------------ the comparator
def compare(bounds, got):
    """bounds {name: Fl}, got {name: tensor of any float dtype} -> {name: max(err / tol)}"""
    rep = {}
    for name, b in bounds.items():
        g = got[name].detach().double().cpu().reshape(b.v.shape)
        if g.numel() == 0:
            rep[name] = 0.0
            continue
        err = (g - b.v).abs()
        ratio = torch.where(b.e > 0, err / b.e.clamp_min(1e-320), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
        rep[name] = float(ratio.max())
    return rep


def merge(worst, rep, prefix=""):
    for k, v in rep.items():
        worst[prefix + k] = max(worst.get(prefix + k, 0.0), v)
    return worst


def own_inputs(got, prec):
    """The PE columns of an fp32 slot against the slot's OWN raw columns (the position the kernel encoded, exact in fp32): only the
    encoder's error is left, sincos_abs per element, however large the rounding of the position was.  {} for bf16 slots (the raw
    columns are rounded copies there) -- and not for the integrated PE, whose variance is not in the slot."""
    if prec != "fp32":
        return {}
    out = {"pos-pe|raw": pe(Fl(got["pos-raw"].double()), 10, "direct")}
    if "dir-raw" in got:
        out["dir-pe|raw"] = pe(Fl(got["dir-raw"].double()), 4, "direct")
    return out


def slot_outputs(ex, ed=None):
    """the reference-order rows of forward_ref.encodings -> the comparator's names"""
    got = {"pos-raw": ex[:, :3], "pos-pe": ex[:, 3:]}
    if ed is not None:
        got["dir-raw"], got["dir-pe"] = ed[:, :3], ed[:, 3:]
    return got


# ------------------------------------------------------------------------------------------------ the inputs
def _unit(n, gen):
    v = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def directions(n, gen):
    """un-normalised, |d| log-uniform in [0.3, 3]; every fifth has a zero component, every eleventh a negative zero"""
    d = _unit(n, gen) * (0.3 * 10.0 ** torch.rand(n, 1, generator=gen, dtype=torch.float64))
    d = d.float()
    d[0::5, 1] = 0.0
    d[3::11, 2] = -0.0
    return d


def ray_batch(N, seed):
    """(N, 6) fp32: origins in [-0.5, 0.5]^3 with coordinates 0, -0 and denormals mixed in by n % 7, `directions`"""
    gen = torch.Generator().manual_seed(seed)
    o = (torch.rand(N, 3, generator=gen) - 0.5)
    o[1::7, 0] = 0.0
    o[2::7, 1] = -0.0
    o[3::7, 2] = 1e-40
    o[4::7, 0] = -3e-42
    return torch.cat((o, directions(N, gen)), -1).contiguous()


DEPTH_FAMILIES = ("workload", "wide", "thin", "degenerate", "geometric")


def depth_rows(rays, S1, families, seed):
    """(N, S1) sorted depths, ray n from family families[n % len(families)]:
      workload    uniform in [NEAR, FAR]
      wide        uniform in disparity between NEAR and FAR_WIDE = 1000
      thin        z_{i+1} = z_i (1 + 2e-4): hw / mid = 1e-4
      degenerate  workload with every odd depth a copy of the one before it: every other frustum has z0 == z1
      geometric   ipe_gaussian_ref's `far` family: 0.2 .. 1e6"""
    gen = torch.Generator().manual_seed(seed)
    N = rays.shape[0]
    srt = lambda: torch.sort(torch.rand(N, S1, generator=gen, dtype=torch.float64), dim=-1)[0]
    rows = {}
    rows["workload"] = NEAR + (FAR - NEAR) * srt()
    s = srt()
    rows["wide"] = 1.0 / ((1 - s) / NEAR + s / FAR_WIDE)
    z0 = NEAR + (FAR - NEAR) * torch.rand(N, 1, generator=gen, dtype=torch.float64)
    rows["thin"] = z0 * (1 + 2e-4) ** torch.arange(S1, dtype=torch.float64)[None, :]
    deg = NEAR + (FAR - NEAR) * srt()
    deg[:, 1::2] = deg[:, 0::2][:, : deg[:, 1::2].shape[1]]
    rows["degenerate"] = deg
    rows["geometric"] = G.depths(rays, S1 - 1, "far", gen).double() if S1 > 1 else rows["workload"]
    z = torch.empty(N, S1, dtype=torch.float64)
    for k, fam in enumerate(families):
        z[k::len(families)] = rows[fam][k::len(families)]
    return z.float().contiguous()


def _ray_gap(rays, z, frusta):
    """per ray: min | |x| - 1 | over its sample positions o + z d and (frusta) the metric means of its frusta"""
    o, d = rays[:, None, :3].double(), rays[:, None, 3:6].double()
    gap = ((o + z.double()[..., None] * d).norm(dim=-1) - 1).abs().min(dim=-1)[0]
    if frusta and z.shape[1] > 1:
        mu_t = cone_moments(z)[0]
        gap = torch.minimum(gap, ((o + mu_t[..., None] * d).norm(dim=-1) - 1).abs().min(dim=-1)[0])
    return gap


def clear_of_sphere(rays, z, frusta=True, scale="z"):
    """Input construction, not an exemption: a ray with a sample (or a frustum mean) within 2 SPHERE_GAP of the unit sphere has its
    depths (scale = "z") or its origin (scale = "o": the depths are not the caller's to move) scaled by 1 + 7e-4 until none is.
    -> (rays, z), new tensors."""
    rays, z = rays.clone(), z.clone()
    for _ in range(200):
        bad = _ray_gap(rays, z, frusta) < 2 * SPHERE_GAP
        if not bool(bad.any()):
            return rays, z
        if scale == "z":
            z[bad] = (z[bad].double() * (1 + 7e-4)).float()
        else:
            rays[bad, :3] = (rays[bad, :3].double() * (1 + 7e-4) + 1e-3).float()
    raise AssertionError("could not move every sample off the unit sphere")


def jittered_depths(z_base, u, z_jitter):
    """the fp32 depths of the z_base + u z_jitter source, as the kernel forms them (for clear_of_sphere only)"""
    return z_base[None, :] + u * torch.tensor(z_jitter, dtype=torch.float32)


def point_batch(M, stride, seed, far):
    """(M, stride) fp32 for mode 0, row m from family m % 8:
      0, 1  the workload's o + z d;  2  coordinates drawn from {0, -0, 1e-40, -3e-42, 0.25, -0.5};  3  just inside |x| = 1 (2e-4 .. 2e-2);
      4  just outside;  5  |x| log-uniform in [10, far];  6  N(0, 1);  7  |x| log-uniform in [1e-6, 1e-2] (raw coordinates near 0)
    columns 3..5 (stride 6): `directions`.  Rows of the random families closer than 2 SPHERE_GAP to the sphere are scaled off it."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.empty(M, 3, dtype=torch.float64)
    r = lambda n: torch.rand(n, 1, generator=gen, dtype=torch.float64)
    n = [len(range(k, M, 8)) for k in range(8)]
    for k in (0, 1):
        x[k::8] = (torch.rand(n[k], 3, generator=gen, dtype=torch.float64) - 0.5) + (NEAR + (FAR - NEAR) * r(n[k])) * directions(n[k], gen).double()
    table = torch.tensor([0.0, -0.0, 1e-40, -3e-42, 0.25, -0.5], dtype=torch.float32)
    special = table[torch.randint(0, 6, (n[2], 3), generator=gen)]
    delta = lambda m: 2e-4 * 100.0 ** r(m)
    x[3::8] = _unit(n[3], gen) * (1 - delta(n[3]))
    x[4::8] = _unit(n[4], gen) * (1 + delta(n[4]))
    x[5::8] = _unit(n[5], gen) * (10.0 * (far / 10.0) ** r(n[5]))
    x[6::8] = torch.randn(n[6], 3, generator=gen, dtype=torch.float64)
    x[7::8] = _unit(n[7], gen) * (1e-6 * 1e4 ** r(n[7]))
    x[2::8] = 0.0
    x = x.float()
    x[2::8] = special
    for _ in range(200):
        bad = ((x.double().norm(dim=-1) - 1).abs() < 2 * SPHERE_GAP)
        bad[3::8] = False
        bad[4::8] = False
        if not bool(bad.any()):
            break
        x[bad] = (x[bad].double() * (1 + 7e-4)).float()
    out = torch.zeros(M, stride, dtype=torch.float32)
    out[:, :3] = x
    if stride >= 6:
        out[:, 3:6] = directions(M, gen)
    if stride > 6:
        out[:, 6:] = 777.0                                   # never read
    return out.contiguous()


def ipe_dn(rays):
    """the fp32 direction norm handed to the integrated-PE kernels in these tests: max(|D|, DN_FLOOR), so that 1 - d_c^2 / dn > 0"""
    return max(f32(float((rays[:, 3:6].double() ** 2).sum().sqrt())), DN_FLOOR)


# ------------------------------------------------------------------------------------------------ the sample descriptors of the tests
SOURCES = ("pts", "pts-wide", "z", "u", "philox", "cam")
PHILOX_SEED = 20240917
CAM_W, CAM_F = 37, 40.0


def ray_split(M):
    """M = N x S with the largest ragged S (a prime below 64, so rays straddle the 32- and 64-sample groups) that divides M"""
    S = next(s for s in (61, 59, 53, 47, 43, 41, 37, 31, 29, 23, 19, 17, 13, 11, 7, 5, 3, 2, 1) if M % s == 0)
    return M // S, S


def sample_gaps(src):
    return (positions(src)[0].v.norm(dim=-1) - 1).abs()


def make_source(kind, net, M, contracted, ipe=False, philox_u=None):
    """The descriptor `kind` of SOURCES with M samples as a dict of CPU tensors (see `positions`), every sample (and, for "z", every
    metric frustum mean) at least 2 SPHERE_GAP from the unit sphere.
      pts        mode 0, stride 3 (proposal) / 6 (fine)            pts-wide   stride 6 / 8
      z          mode 1, explicit depths, z_stride = S + 3 > S     (the only kind the integrated PE accepts: S + 1 depths are read)
      u          mode 1, z_base + u z_jitter with u a tensor       philox     the same, u = the stratified Philox stream of PHILOX_SEED
      cam        mode 2: directions from cx, cy and the pose, depths as in "u"
    The geometric depth family (to 1e6) and |x| up to 1e6 enter only with the contraction; without it the far family stops at 1000."""
    seed = 7919 * SOURCES.index(kind) + M + (1 if contracted else 0)
    if kind in ("pts", "pts-wide"):
        stride = {"pts": 3, "pts-wide": 6}[kind] if net == "prop" else {"pts": 6, "pts-wide": 8}[kind]
        return {"mode": 0, "pts": point_batch(M, stride, seed, 1e6 if contracted else FAR_WIDE * 3.0)}
    N, S = ray_split(M)
    gen = torch.Generator().manual_seed(seed)
    if kind == "z":
        rays = ray_batch(N, seed)
        fams = DEPTH_FAMILIES if contracted else DEPTH_FAMILIES[:4]
        z = depth_rows(rays, S + 1, fams, seed + 1)
        rays, z = clear_of_sphere(rays, z, frusta=True)
        zz = torch.full((N, S + 3), 1e30)
        zz[:, : S + 1] = z
        return {"mode": 1, "rays": rays, "S": S, "z": zz.contiguous()}
    z_base = torch.linspace(NEAR, FAR, S)
    jitter = (FAR - NEAR) / S
    if kind == "philox":
        u = philox_u(PHILOX_SEED, N, S)
        rays = ray_batch(N, seed)
        rays, _ = clear_of_sphere(rays, jittered_depths(z_base, u, jitter), frusta=False, scale="o")
        return {"mode": 1, "rays": rays, "S": S, "z_base": z_base, "u": u, "z_jitter": jitter, "seed": PHILOX_SEED}
    u = torch.rand(N, S, generator=gen)
    if kind == "u":
        src = {"mode": 1, "rays": ray_batch(N, seed), "S": S, "z_base": z_base, "u": u, "z_jitter": jitter}
    else:
        from oracle import nerf_oracle as O
        pose = [float(v) for v in O.pose_spherical(30.0, -30.0, 4.0)[:3].reshape(-1).float()]
        src = {"mode": 2, "pose": pose, "H": (N + CAM_W - 1) // CAM_W, "W": CAM_W, "fx": CAM_F, "fy": CAM_F * 1.25, "N": N, "S": S,
               "z_base": z_base, "u": u, "z_jitter": jitter}
    for _ in range(200):
        bad = (sample_gaps(src) < 2 * SPHERE_GAP).reshape(N, S)
        if not bool(bad.any()):
            return src
        u[bad] = (u[bad] + 0.37) % 1.0
    raise AssertionError("could not move every sample off the unit sphere")


def radius_r2(r):
    """the fp32 r2 the entry points hand the kernels: (float)((double)(float)r * (double)(float)r)"""
    r32 = f32(r)
    return f32(r32 * r32)
