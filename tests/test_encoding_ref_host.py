"""tests/encoding_ref.py checked on the CPU before it is trusted as a yardstick (no GPU):

  1. the specification against the oracle (fp64) and the goldens g03_pe, g12_ipe, g18_ipe_l10; the contraction against
     generic_ref.contract_spec;
  2. sin_quadrant / sincos_quadrant restated operation by operation in fp32 (an FMA = the fp64 product and sum rounded once to fp32):
     the |k|-dependent bound of ipe_gaussian_ref (SIN_QUADRANT) holds over a dense sweep up to 2^21, next to multiples of pi/2 and next
     to half-integers of a 2/pi; the constants of the derivation in exact rational arithmetic; the polynomial sup re-measured;
  3. an fp32 emulation of the kernels' sequences -- direct path, doubling path, bf16 store -- inside every bound on exactly the inputs
     the GPU test uses (encoding_ref.make_source and the stand-alone constructors), worst err/tol printed per output;
  4. fourteen planted faults, each reported by the comparator;
  5. two of them pass the old whole-tensor gates (1e-6 max for the cone parameters) while the comparator reports them."""
import math
from decimal import Decimal
from fractions import Fraction

import pytest
import torch

import encoding_ref as E
import generic_ref as GR
import ipe_gaussian_ref as G
from oracle import nerf_oracle as O

U = E.U
RADIUS = 2.0 / 12.0 ** 0.5 / 55.0
R2 = E.radius_r2(RADIUS)
TILE = {"bf16": 256, "fp32": 128}


def _t(v):
    return torch.tensor(v, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ device_common.h restated in fp32
C0, C1, C2, C3 = _t(0.6366197466850281), _t(1.57079637050628662109375), _t(-4.371138828673793e-08), _t(-1.7151245100058819e-15)
PS = [_t(v) for v in (1.5896910177e-10, -2.5050759689e-08, 2.7557314297e-06, -1.9841270114e-04, 8.3333337680e-03, -1.6666667163e-01)]
PC = [_t(v) for v in (-1.1359647598e-11, 2.0875723372e-09, -2.7557314297e-07, 2.4801587642e-05, -1.3888889225e-03, 4.1666667908e-02)]


def fmaf(a, b, c):
    return (a.double() * b.double() + torch.as_tensor(c).double()).float()


def _reduce(a):
    k = torch.round(a * C0)                                           # rintf: half to even
    r = fmaf(-k, C1, a)
    r = fmaf(-k, C2, r)
    r = fmaf(-k, C3, r)
    return k, r


def _kernels(r):
    z = r * r
    ps = fmaf(z, PS[0], PS[1])
    for c in PS[2:]:
        ps = fmaf(z, ps, c)
    s = fmaf(r * z, ps, r)
    pc = fmaf(z, PC[0], PC[1])
    for c in PC[2:]:
        pc = fmaf(z, pc, c)
    c = fmaf(z * z, pc, fmaf(_t(-0.5), z, _t(1.0)))
    return s, c


def sin_quadrant(a, quad):
    k, r = _reduce(a)
    n = k.to(torch.int64) + quad
    s, c = _kernels(r)
    v = torch.where((n & 1) != 0, c, s)
    return torch.where((n & 2) != 0, -v, v)


def sincos_quadrant(a):
    k, r = _reduce(a)
    n = k.to(torch.int64)
    s, c = _kernels(r)
    vs, vc = torch.where((n & 1) != 0, c, s), torch.where((n & 1) != 0, s, c)
    return torch.where((n & 2) != 0, -vs, vs), torch.where(((n + 1) & 2) != 0, -vc, vc)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 2: the reduction
def _sweep():
    """fp32 arguments up to 2^21: log-spaced, the fp32 neighbours of multiples of pi/2, and of half-integers of a 2/pi (where k may be
    the other neighbour), of both signs; the special values"""
    gen = torch.Generator().manual_seed(3)
    logs = (2.0 ** (torch.rand(400000, generator=gen, dtype=torch.float64) * 47 - 26)).float()
    k = torch.cat((torch.arange(0, 4096, dtype=torch.float64), torch.round(2.0 ** (torch.rand(60000, generator=gen, dtype=torch.float64) * 9.3 + 12))))
    k = k[k * (math.pi / 2) < 2.0 ** 21 - 4]
    parts = [logs]
    for centre in (k * (math.pi / 2), (k + 0.5) * (math.pi / 2)):
        c = centre.float()
        for step in range(-3, 4):
            v = c.clone()
            for _ in range(abs(step)):
                v = torch.nextafter(v, torch.full_like(v, float("inf") if step > 0 else -float("inf")))
            parts.append(v)
    a = torch.cat(parts + [_t([0.0, -0.0, 1e-40, -3e-42, 2.0 ** 21, 1.0, 0.78539816, 0.785398185])])
    a = a[a.abs() <= 2.0 ** 21]
    return torch.cat((a, -a))


def test_constants_of_the_reduction_in_exact_arithmetic():
    half_pi = Fraction(Decimal("1.57079632679489661923132169163975144209858469968755291048747"))
    c1, c2, c3, c0 = (Fraction(float(c)) for c in (C1, C2, C3, C0))
    rho = abs(half_pi - c1 - c2 - c3)
    eps0 = abs(c0 * half_pi - 1)
    print("rho = %.4e (2^%.2f)   e0 = %.6e   |pi/2 - C1| = %.4e" % (float(rho), math.log2(float(rho)), float(eps0), float(abs(half_pi - c1))))
    assert rho <= Fraction(G.SINCOS_RHO)
    assert float(eps0) * (1 + U) + U <= G.SINCOS_ETA * (1 + 1e-12) and G.SINCOS_ETA < 1.0e-7
    assert float(abs(half_pi - c1)) < 4.38e-8 and float(c1) * 2 ** 23 == int(float(c1) * 2 ** 23)
    # the documented figures, and where the constant 4 u stops being covered by the derivation
    d = lambda a: float(G.sincos_derived(torch.tensor(a, dtype=torch.float64))) / U
    print("D = %.3f u at 2^15, %.3f u at 1.536e6, %.3f u at 2^21, %.3f u at 2^21.1" % (d(2.0 ** 15), d(1.536e6), d(2.0 ** 21), d(2.0 ** 21.1)))
    assert d(2.0 ** 15) < 3.62 and d(1.536e6) < 3.89 and d(2.0 ** 21) <= 4.0 < d(2.0 ** 21.1)
    assert float(G.sincos_reduced_range(torch.tensor(2.0 ** 21, dtype=torch.float64))) < G.POLY_RANGE
    with pytest.raises(AssertionError, match="beyond 2\\^21"):
        G.sincos_abs(G.Fl(torch.tensor([2.0 ** 21 + 1], dtype=torch.float64)))


def test_polynomial_sup_is_inside_its_allowance():
    r = torch.linspace(-G.POLY_RANGE, G.POLY_RANGE, 2000001, dtype=torch.float64)
    z = r * r
    ps = PS[0].double()
    for c in PS[1:]:
        ps = ps * z + c.double()
    pc = PC[0].double()
    for c in PC[1:]:
        pc = pc * z + c.double()
    es, ec = float((r + r * z * ps - torch.sin(r)).abs().max()), float((z * z * pc + (1 - 0.5 * z) - torch.cos(r)).abs().max())
    print("sup |P_s - sin| = %.3f u, sup |P_c - cos| = %.3f u on |r| <= %.1f; allowed %.2f u" % (es / U, ec / U, G.POLY_RANGE, G.POLY_APPROX / U))
    assert max(es, ec) <= G.POLY_APPROX / 1.9


def test_reduction_bound_holds_for_the_emulated_sin_quadrant():
    a = _sweep()
    k, r = _reduce(a)
    a64 = a.double()
    # the steps of the derivation: the first FMA is exact, |r| stays inside R(q), k is one of the two neighbours
    assert torch.equal(fmaf(-k, C1, a).double(), a64 - k.double() * C1.double())
    R = G.sincos_reduced_range(a64.abs())
    assert bool((r.double().abs() <= R * (1 + 2.0 ** -20)).all())
    assert bool(((a64 * (2 / math.pi) - k.double()).abs() <= 0.5 + G.SINCOS_ETA * a64.abs() * (2 / math.pi)).all())
    off = int(((a64 * (2 / math.pi) - k.double()).abs() > 0.5).sum())
    assert off > 0, "the sweep never reached a k off by one"
    assert float(r.double().abs().max()) > math.pi / 4
    # the reduced argument against a - k pi/2 (the three constants carry pi/2 to 2^-72: fp64 cannot hold that difference, Fraction can on a sample)
    idx = torch.linspace(0, a.numel() - 1, 3000).long()
    half_pi = Fraction(Decimal("1.57079632679489661923132169163975144209858469968755291048747"))
    worst_red = 0.0
    for i in idx.tolist():
        exact = Fraction(float(a[i])) - Fraction(float(k[i])) * half_pi
        q = abs(float(a[i])) * 2 / math.pi
        tol = 2 * U * float(R[i]) * (1 + 2.0 ** -20) + (q * (1 + G.SINCOS_ETA) + 0.5) * G.SINCOS_RHO
        worst_red = max(worst_red, float(abs(Fraction(float(r[i])) - exact)) / tol)
    sn, cs = sincos_quadrant(a)
    assert torch.equal(_bits(sn), _bits(sin_quadrant(a, 0))) and torch.equal(_bits(cs), _bits(sin_quadrant(a, 1)))
    bound = G.sincos_derived(a64.abs())
    es, ec = (sn.double() - torch.sin(a64)).abs(), (cs.double() - torch.cos(a64)).abs()
    print("sin_quadrant over %d arguments up to 2^21 (%d with k off by one): reduction %.3f of its bound; sin %.3f, cos %.3f of D(|a|); "
          "worst %.3f u, %.3f u" % (a.numel(), off, worst_red, float((es / bound).max()), float((ec / bound).max()), float(es.max()) / U, float(ec.max()) / U))
    assert worst_red <= 1.0
    assert float((es / bound).max()) <= 1.0 and float((ec / bound).max()) <= 1.0
    assert float(torch.maximum(es, ec).max()) <= G.SINCOS_ABS          # inside the domain the constant stands as well
    assert sin_quadrant(_t([-0.0]), 0).item() == 0.0 and sincos_quadrant(_t([1e-40]))[0].item() == _t(1e-40).item()


def test_doubling_chain_error_grows_faster_than_the_angle():
    """The bf16 kernels' comment promises an octave-9 error of 2^9 . 1e-7 = 5e-5: the growth of an ANGLE error.  The recurrence
    also moves the point (s, c) off the unit circle, and that radial error eps goes to 4 eps sin^2(theta) per step -- a factor 3 at every
    step on the orbit 2 pi / 3 <-> 4 pi / 3.  The fp32 emulation on a million arguments in [-8, 8] shows it (about 2e4 u = 1.3e-3 at
    octave 9) and stays inside the derived bound, which allows a factor 4 per step."""
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(1000000, 1, generator=gen) * 16 - 8).expand(-1, 3).contiguous()
    got = _pe32(x, 10, "doubling").double()
    b = E.pe(E.Fl(x.double()), 10, "doubling")
    err = (got - b.v).abs()
    worst9 = float(err[:, 54:].max())
    print("doubling chain, fp32 emulation: octave-9 error %.3e = %.0f u (2^9 u = %.1e, 3^9 u = %.1e, derived bound up to %.1e); err/tol %.3f"
          % (worst9, worst9 / U, 512 * U, 19683 * U, float(b.e[:, 54:].max()), float((err / b.e).max())))
    assert float((err / b.e).max()) <= 1.0
    assert worst9 > 10 * 2.0 ** 9 * 1e-7                    # an order of magnitude beyond the comment's figure
    assert worst9 < 2.0 ** -9                               # ... and still below the bf16 half-ulp of a feature of size 1/2 .. 1


# ------------------------------------------------------------------------------------------------ 1: the specification
def test_specification_against_the_oracle_and_the_goldens(golden):
    g = golden("g03_pe")
    for x, L, want in ((g["x"], 10, g["pe10"]), (g["x"], 4, g["pe4"]), (g["x2d"], 4, g["pe4_2d"])):
        x = x.reshape(-1, 3)
        for path in ("direct", "doubling", "libm", "libm-doubling"):
            got = E.pe(E.Fl(x.double()), L, path).v
            assert float((got - O.positional_encoding(x.double(), L)).abs().max()) < 1e-12, path
            assert float((got - want.reshape(-1, 6 * L).double()).abs().max()) < 2e-6, path          # (the golden is the reference's fp32)
    r, r2 = 2.0 ** -10, 2.0 ** -20
    for name, L in (("g12_ipe", 6), ("g18_ipe_l10", 10)):
        g = golden(name)
        z, rays = g["z"], g["rays"]
        dn = E.f32(float(rays[:, 3:].double().norm()))
        for mode, contracted in (("plain", False), ("metric", True)):
            want = O.ipe_feature(z.double(), rays.double(), L, r, dir_norm=torch.tensor(dn, dtype=torch.float64), contracted=contracted)
            feat, mu, _ = G.spec(z, rays, L, r2, dn, mode=mode)
            assert float((feat - want[0]).abs().max()) < 1e-12 and float((mu - want[1]).abs().max()) < 1e-12, (name, mode)
            for path in ("direct", "doubling"):
                b = E.ipe(z, rays, L, r2, dn, mode, path)
                assert float((b["pe"].v - want[0].reshape(-1, 6 * L)).abs().max()) < 1e-9 and float((b["raw"].v - want[1].reshape(-1, 3)).abs().max()) < 1e-12
            cp = E.cone_parameters(z, r2)
            for a, b in zip((cp["mu_t"].v, cp["var_t"].v, cp["var_r"].v), O.cone_parameters(z.double(), r)):
                assert float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) < 1e-9
        # the goldens themselves are the reference's own fp32 run (its radius, its direction norm) of the same sequence of operations:
        # inside the derived bounds of the direct path, element by element
        rad = 0.0015 if name == "g12_ipe" else float(g["radius"])
        dn = float(g["dir_norm"]) if name == "g18_ipe_l10" else dn
        rep = E.compare(E.ipe(z, rays, L, E.radius_r2(rad), dn, "plain"), {"pe": g["feat"], "raw": g["mu"]})
        cp = E.cone_parameters(z, E.radius_r2(rad))
        rep["mu_t"] = E.compare({"mu_t": cp["mu_t"]}, g)["mu_t"]
        if name == "g18_ipe_l10":
            rep.update(E.compare({k: cp[k] for k in ("var_t", "var_r")}, g))
        print("golden %s inside the derived bounds: %s" % (name, rep))
        assert max(rep.values()) <= 1.0, (name, rep)


def test_contraction_is_generic_refs():
    x = E.point_batch(4001, 3, 5, 1e6)
    got, gap = E.contract(E.Fl(x.double()))
    want, _ = GR.contract_spec(x)
    assert gap >= E.SPHERE_GAP
    assert float(((got.v - want).abs() / want.abs().clamp_min(1e-300)).max()) < 1e-14
    n = x.double().norm(dim=-1)
    assert bool(((n > 1) & (n < 1.001)).any()) and bool(((n < 1) & (n > 0.999)).any()) and bool((n > 1e5).any()) and bool((n == 0).any())


# ------------------------------------------------------------------------------------------------ 3: the fp32 emulation
def _norm3(v):
    return ((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3]).sqrt()


def _contract32(x, fault=None):
    n = _norm3(x)
    k = (2.0 - 1.0 / n) / n
    take = (n < 1.0) if fault == "inside" else (n > 1.0)
    return torch.where(take, x * k, x)


def _bf16(t, fault=None):
    if fault == "trunc":
        return (_bits(t) & -65536).view(torch.float32)
    return t.bfloat16().float()


def _pe32(x, L, path, fault=None):
    """x (M, 3) fp32 -> (M, 6 L): path direct / doubling / libm / libm-doubling"""
    libm = path.startswith("libm")
    first = (lambda a: (torch.sin(a), torch.cos(a))) if libm else sincos_quadrant
    out = []
    if path in ("direct", "libm"):
        for l in range(L):
            scale = 2.0 ** (L - 2) if (fault == "octave" and l == L - 1) else 2.0 ** l
            s, c = first(x * _t(scale))
            out += [c, s] if (fault == "swap" and l == 1) else [s, c]
    else:
        s, c = first(x)
        for l in range(L):
            out += [s, c]
            if fault == "doubling" and l == L - 2:
                continue
            s2 = 2.0 * s
            s, c = s2 * c, fmaf(-s2, s, _t(1.0))
    return torch.cat(out, -1)


def _positions32(src, fault=None):
    if src["mode"] == 0:
        p = src["pts"]
        return p[:, :3].clone(), (p[:, 3:6].clone() if p.shape[1] >= 6 else None)
    S = src["S"]
    if src["mode"] == 1:
        o, d = src["rays"][:, None, :3], src["rays"][:, None, 3:6]
        N = src["rays"].shape[0]
    else:
        N, W, H = src["N"], src["W"], src["H"]
        n = torch.arange(N)
        row, cl = (n // W).float(), (n % W).float()
        cx = ((cl - _t(float(W)) * 0.5) + 0.5) / _t(src["fx"])
        cy = ((_t(float(H)) * 0.5 - row) + 0.5) / _t(src["fy"])
        P = [_t(v) for v in src["pose"]]
        d = torch.stack([(cx * P[4 * c] + cy * P[4 * c + 1]) + (-1.0) * P[4 * c + 2] for c in range(3)], -1)[:, None, :]
        o = torch.stack((P[3], P[7], P[11]))[None, None, :]
    if src.get("z") is not None:
        z = src["z"].reshape(-1)[: N * S].reshape(N, S) if fault == "zstride" else src["z"][:, :S]
    else:
        z = src["z_base"][None, :] + src["u"] * _t(src["z_jitter"])
    x = o + z[..., None] * d
    return x.reshape(N * S, 3), d.expand(N, S, 3).reshape(N * S, 3)


def _ipe32(z, rays, L, r2, dn, mode, path, fault=None):
    z0, z1 = z[:, :-1, None], z[:, 1:, None]
    r2, dn = _t(r2), _t(1.0 if fault == "dn1" else dn)
    c512 = _t(0.4 if fault == "0.4" else G.FIVE_TWELFTHS_F32)
    mid, hw = (z1 + z0) / 2, (z1 - z0) / 2
    hw2, mid2 = hw * hw, mid * mid
    t1 = 3 * mid2 + hw2
    mu_t = mid if fault == "mid" else mid + ((2 * mid) * hw2) / t1
    hw4 = hw2 * hw2
    var_t = hw2 / 3 - (((4 * hw4) * (12 * mid2 - hw2)) / 15) / (t1 * t1)
    var_r = r2 * ((0.25 * mid2 + c512 * hw2) - (4 * hw4) / (15 * t1))
    o, d = rays[:, None, :3], rays[:, None, 3:6]
    mu = o + mu_t * d
    dd = d * d
    var = var_t * dd + var_r * (1 - dd / dn)
    if mode == "metric" and fault != "uncontracted":
        mu = _contract32(mu)
    M = mu.shape[0] * mu.shape[1]
    mu, var = mu.reshape(M, 3), var.reshape(M, 3)
    out = []
    if path == "direct":
        for l in range(L):
            s, c = sincos_quadrant(mu * _t(2.0 ** l))
            e = torch.exp(-0.5 * (var * _t((2.0 if fault == "att2l" else 4.0) ** l)))
            out += [s * e, c * e]
    else:
        (s, c), at = sincos_quadrant(mu), torch.exp(-0.5 * var)
        for l in range(L):
            out += [s * at, c * at]
            s2 = 2.0 * s
            s, c = s2 * c, fmaf(-s2, s, _t(1.0))
            a2 = at * at
            at = a2 * a2 if fault != "att2l" else a2
    return {"pe": torch.cat(out, -1), "raw": mu}, {"mu_t": mu_t[..., 0], "var_t": var_t[..., 0], "var_r": var_r[..., 0]}


def _fused32(src, net, prec, contracted, ipe_args=None, fault=None):
    bf16 = prec == "bf16"
    path = "doubling" if bf16 else "direct"
    store = (lambda t: _bf16(t, fault)) if bf16 else (lambda t: t)
    x, d = _positions32(src, fault)
    if ipe_args is not None:
        got, _ = _ipe32(src["z"][:, : src["S"] + 1].contiguous(), src["rays"], 10, ipe_args[0], ipe_args[1], "metric" if contracted else "plain", path, fault)
        raw, feat = got["raw"], got["pe"]
    else:
        if contracted:
            x = _contract32(x, fault)
        raw, feat = x, _pe32(x, 10, path, fault)
    if fault == "yz":
        raw = raw[:, [0, 2, 1]]
    out = {"pos-raw": store(raw), "pos-pe": store(feat)}
    if net == "mip":
        dh = d if fault == "nonorm" else d / _norm3(d)
        out["dir-raw"], out["dir-pe"] = store(dh), store(_pe32(dh, 4, path))
    return out


def _encode_rows32(x, L, normalize, bf16, fault=None):
    x = x[:, :3]
    if normalize:
        x = x / _norm3(x)
    feat = _pe32(x, L, "libm-doubling" if bf16 else "libm", fault)
    pad = torch.zeros(x.shape[0], (3 + 6 * L + 7) // 8 * 8 - 3 - 6 * L)
    if fault == "pad":
        pad[x.shape[0] // 2, 0] = 1e-30
    store = _bf16 if bf16 else (lambda t: t)
    return {"raw": store(x), "pe": store(feat), "pad": pad}


FUSED_CASES = [(net, prec, kind) for net in ("prop", "mip") for prec in ("fp32", "bf16") for kind in E.SOURCES]


def _philox_u(seed, N, S):
    return O.philox_uniforms(seed, N, 0, S, 1)[0]


def _report(title, worst):
    print("%-44s %s" % (title, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, "%s: the fp32 emulation leaves the bound in %s" % (title, bad)


@pytest.mark.parametrize("net,prec,kind", FUSED_CASES)
def test_emulation_of_the_fused_kernels_is_inside_every_bound(net, prec, kind):
    """the descriptors of tests/test_gpu_encoding.py at the two small sample counts (the large one differs only in length)"""
    worst = {}
    for contracted in (False, True):
        for M in (TILE[prec] - 1, TILE[prec] + 1, 3 * TILE[prec] + 77):
            src = E.make_source(kind, net, M, contracted, philox_u=_philox_u)
            b, gap = E.fused(src, net, prec, contracted)
            assert not contracted or gap >= E.SPHERE_GAP, gap
            got = _fused32(src, net, prec, contracted)
            E.merge(worst, E.compare(b, got))
            E.merge(worst, E.compare(E.own_inputs(got, prec), {"pos-pe|raw": got["pos-pe"], "dir-pe|raw": got.get("dir-pe")}))
            if kind == "z" and net == "mip":
                dn = E.ipe_dn(src["rays"])
                b, gap = E.fused(src, net, prec, contracted, ipe_args=(R2, dn))
                assert not contracted or gap >= E.SPHERE_GAP, gap
                E.merge(worst, E.compare(b, _fused32(src, net, prec, contracted, ipe_args=(R2, dn))), "ipe-")
    _report("fused %s %s %s" % (net, prec, kind), worst)


def standalone_inputs(M, seed, wide=True):
    """positions for the stand-alone encoders: point_batch out to 3000 (the octave-9 argument reaches 1.54e6)"""
    return E.point_batch(M, 6, seed, E.FAR_WIDE * 3.0 if wide else 8.0)


def test_emulation_of_the_stand_alone_encoders_is_inside_every_bound():
    worst = {}
    for L in (1, 4, 10):
        for M in (1, 63, 64, 65, 333):
            x = standalone_inputs(M, 100 + M)[:, :3].contiguous()
            E.merge(worst, E.compare({"pe": E.pe(E.Fl(x.double()), L, "direct")}, {"pe": _pe32(x, L, "direct")}), "pe_kernel ")
    for L in (4, 10):
        for normalize in (False, True):
            for bf16 in (False, True):
                x = standalone_inputs(333, 7 + L)
                x = x[:, 3:6] if normalize else x[:, :3]
                E.merge(worst, E.compare(E.encode_rows(x, L, normalize, bf16), _encode_rows32(x, L, normalize, bf16)), "encode_rows %s " % ("bf16" if bf16 else "fp32"))
    for L in (6, 10):
        for S in (1, 7, 128):
            for contracted in (False, True):
                rays, z = _ipe_inputs(9, S, contracted)
                dn = E.ipe_dn(rays)
                mode = "metric" if contracted else "plain"
                got, cp = _ipe32(z, rays, L, R2, dn, mode, "direct")
                E.merge(worst, E.compare(E.ipe(z, rays, L, R2, dn, mode), got), "ipe_feature %s " % mode)
                E.merge(worst, E.compare(E.cone_parameters(z, R2), cp), "cone ")
    for N in (1, 1023, 1025):
        rays = E.ray_batch(N, N)
        E.merge(worst, E.compare(E.dirs_norm(rays), {"dn": (rays[:, 3:6].double() ** 2).sum().sqrt().float()}))
        dh = rays[:, 3:6] / _norm3(rays[:, 3:6])
        E.merge(worst, E.compare(E.direction_table(rays), {"dir-raw": _bf16(dh), "dir-pe": _bf16(_pe32(dh, 4, "doubling"))}), "table ")
    _report("stand-alone encoders", worst)


def _ipe_inputs(N, S, contracted, seed=0):
    rays = E.ray_batch(N, 50 + N + S + seed)
    z = E.depth_rows(rays, S + 1, E.DEPTH_FAMILIES if contracted else E.DEPTH_FAMILIES[:4], 60 + S + seed)
    return E.clear_of_sphere(rays, z)


# ------------------------------------------------------------------------------------------------ 4: planted faults
def _ratio(rep):
    return max(rep.values())


def test_every_planted_fault_is_reported():
    M = 333
    seen = {}

    def fused_fault(fault, net, prec, kind, contracted, ipe=False):
        src = E.make_source(kind, net, M if kind.startswith("pts") else 7 * 47, contracted, philox_u=_philox_u)
        args = (R2, E.ipe_dn(src["rays"])) if ipe else None
        b, _ = E.fused(src, net, prec, contracted, ipe_args=args)
        honest = _ratio(E.compare(b, _fused32(src, net, prec, contracted, ipe_args=args)))
        seen[fault] = (honest, _ratio(E.compare(b, _fused32(src, net, prec, contracted, ipe_args=args, fault=fault))))

    fused_fault("swap", "prop", "fp32", "pts", False)                   # sin and cos swapped at one octave
    fused_fault("octave", "prop", "fp32", "u", False)                   # last octave scaled by 2^(L-2)
    fused_fault("att2l", "mip", "fp32", "z", False, ipe=True)           # 4^l -> 2^l in the attenuation
    fused_fault("doubling", "prop", "bf16", "pts", True)                # one doubling too few
    fused_fault("trunc", "mip", "bf16", "pts", False)                   # truncating bf16 conversion
    fused_fault("zstride", "prop", "fp32", "z", False)                  # z_stride read as S
    fused_fault("nonorm", "mip", "fp32", "z", False)                    # direction not normalised
    fused_fault("uncontracted", "mip", "fp32", "z", True, ipe=True)     # mean left uncontracted
    fused_fault("inside", "prop", "fp32", "pts", True)                  # contraction applied for n < 1
    fused_fault("mid", "mip", "fp32", "z", False, ipe=True)             # mu_t replaced by mid
    fused_fault("dn1", "mip", "fp32", "z", False, ipe=True)             # dn = 1
    fused_fault("yz", "prop", "bf16", "cam", False)                     # raw slots y and z swapped
    rays, z = _ipe_inputs(9, 128, False)
    b = E.cone_parameters(z, R2)                                        # 5/12 -> 0.4 in var_r
    seen["0.4"] = (_ratio(E.compare(b, _ipe32(z, rays, 10, R2, 16.0, "plain", "direct")[1])),
                   _ratio(E.compare(b, _ipe32(z, rays, 10, R2, 16.0, "plain", "direct", fault="0.4")[1])))
    x = standalone_inputs(M, 3)[:, :3]                                  # a non-zero padding feature
    b = E.encode_rows(x, 10, False, True)
    seen["pad"] = (_ratio(E.compare(b, _encode_rows32(x, 10, False, True))), _ratio(E.compare(b, _encode_rows32(x, 10, False, True, fault="pad"))))
    for fault, (honest, faulty) in seen.items():
        print("fault %-13s honest %.3f   planted %.3g" % (fault, honest, faulty))
    assert len(seen) == 14
    assert all(h <= 1.0 for h, _ in seen.values()), seen
    assert all(f > 1.0 for _, f in seen.values()), seen


# ------------------------------------------------------------------------------------------------ 5: what the old gates cannot see
def test_old_whole_tensor_gates_pass_two_faults_the_comparator_reports():
    """test_gpu_parity's gates on the cone parameters: max |err| <= 1e-6 max |want| over the whole tensor.  128 regular frusta over
    [2, 6] (hw = 1/64) and, for mu_t, frusta with hw / mid = 1e-3."""
    N, S = 9, 128
    rays = E.ray_batch(N, 1)
    z = torch.linspace(2.0, 6.0, S + 1)[None, :].repeat(N, 1).contiguous()
    want = O.cone_parameters(z.double(), E.f32(RADIUS))
    b = E.cone_parameters(z, R2)
    old = lambda got, w: float((got.double() - w).abs().max()) / (1e-6 * float(w.abs().max()))
    faulty = _ipe32(z, rays, 10, R2, 16.0, "plain", "direct", fault="0.4")[1]
    r_old, r_new = old(faulty["var_r"], want[2]), E.compare(b, faulty)["var_r"]
    print("5/12 -> 0.4 in var_r: old gate at %.3f of its limit (passes), comparator at %.3g (reports)" % (r_old, r_new))
    assert r_old <= 1.0 < r_new
    z = (2.0 * (1 + 2e-3) ** torch.arange(S + 1, dtype=torch.float64))[None, :].repeat(N, 1).float().contiguous()
    want = O.cone_parameters(z.double(), E.f32(RADIUS))
    b = E.cone_parameters(z, R2)
    faulty = _ipe32(z, rays, 10, R2, 16.0, "plain", "direct", fault="mid")[1]
    honest = _ipe32(z, rays, 10, R2, 16.0, "plain", "direct")[1]
    r_old, r_new = old(faulty["mu_t"], want[0]), E.compare(b, faulty)["mu_t"]
    print("mu_t -> mid: old gate at %.3f of its limit (passes), comparator at %.3g (reports)" % (r_old, r_new))
    assert r_old <= 1.0 < r_new and max(E.compare(b, honest).values()) <= 1.0
