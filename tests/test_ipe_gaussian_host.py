"""The contracted frustum Gaussian of the integrated PE, host side (no GPU): tests/ipe_gaussian_ref.py's closed form against autograd, its
agreement with the oracle inside the unit ball, var' <= var, an honest fp32 emulation inside the derived bounds and four planted faults
outside them, the `ipe_cov` argument errors of the Python layer, the new symbol and the C-ABI's refusals (which answer before any HIP
call)."""
import ctypes as C
import inspect
import os

import pytest
import torch

import ipe_gaussian_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2 = 2.0 ** -20                                       # a pixel radius of 2^-10: its square is exact in fp32 and in fp64


@pytest.fixture(scope="module")
def inputs():
    rays, zs, _ = G.make_inputs(33, 32, seed=0)
    dn = float(rays[:, 3:].double().norm().float())
    return rays, zs, dn


# ------------------------------------------------------------------------------------------------ the definition
def test_closed_form_is_the_jacobian_push_forward():
    """J Sigma J^T with J = d contract / dx from autograd, Sigma the FULL matrix: its diagonal is the closed form (200 cases, |x| from
    0.1 to 1e3; inside the ball J = I and the diagonal is the metric one)"""
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for i in range(200):
        n = 10.0 ** (-1 + 4 * i / 199.0)
        x = torch.randn(3, generator=gen, dtype=torch.float64)
        x = x / x.norm() * n
        if abs(n - 1) < 1e-3:
            continue
        d = torch.randn(3, generator=gen, dtype=torch.float64)
        var_t, var_r = (torch.rand(2, generator=gen, dtype=torch.float64) + 0.01).tolist()
        dn = float(d.dot(d)) * (1.5 + float(torch.rand(1, generator=gen)))
        sigma = (var_t - var_r / dn) * torch.outer(d, d) + var_r * torch.eye(3, dtype=torch.float64)
        J = torch.autograd.functional.jacobian(lambda p: G.contract(p[None])[0], x)
        want = torch.diagonal(J @ sigma @ J.t())
        vt, vr = torch.tensor([[[var_t]]], dtype=torch.float64), torch.tensor([[[var_r]]], dtype=torch.float64)
        got = G.pushed_variance(x[None, None], d[None, None], vt, vr, dn)[0, 0] if n > 1 else torch.diagonal(sigma)
        worst = max(worst, float(((got - want).abs() / want.abs()).max()))
    assert worst < 1e-11, worst            # (fp64: k d and a x (x.d) cancel to a relative 1e-16 n along the ray)


def test_inside_the_ball_it_is_the_oracle_and_the_variance_never_grows(inputs):
    from oracle import nerf_oracle as O
    rays, zs, dn = inputs
    r = 2.0 ** -10
    for fam, z in zs.items():
        feat, mu, var = G.spec(z, rays, 10, R2, dn)
        feat_m, mu_m, var_m = G.spec(z, rays, 10, R2, dn, mode="metric")
        want = O.ipe_feature(z.double(), rays.double(), 10, r, dir_norm=torch.tensor(dn, dtype=torch.float64), contracted=True)
        assert torch.equal(feat_m, want[0]) and torch.equal(mu_m, want[1]), fam       # the earlier definition, to the bit
        inside = (rays[:, None, :3].double() + want[2][..., None] * rays[:, None, 3:].double()).norm(dim=-1) <= 1
        assert torch.equal(feat[inside], want[0][inside]) and torch.equal(mu, mu_m), fam
        assert bool(inside.all()) == (fam == "inside") and (fam == "inside" or bool((~inside).any())), fam
        # tr(J Sigma J^T) = tr(J^2 Sigma) <= tr(Sigma): the SUM over the coordinates never grows (a single coordinate may -- see the
        # module docstring of ipe_gaussian_ref -- unless the ray passes through the origin, where J and Sigma commute)
        assert bool((var.sum(-1) <= var_m.sum(-1) * (1 + 1e-12)).all()) and bool((var > 0).all()), fam
        assert bool((G.att2(feat, 10).prod(-1) >= G.att2(feat_m, 10).prod(-1) * (1 - 1e-9)).all()), fam
        rad = G.radial(rays)
        feat0, _, var0 = G.spec(z, rad, 10, R2, dn)
        feat0_m, _, var0_m = G.spec(z, rad, 10, R2, dn, mode="metric")
        assert bool((var0 <= var0_m * (1 + 1e-12)).all()), fam
        assert bool((feat0.abs() >= feat0_m.abs() * (1 - 1e-9)).all()), fam
        if fam != "inside":
            assert bool((var[~inside] < 0.9 * var_m[~inside]).any()), fam
            assert bool((var > var_m * (1 + 1e-6)).any()), fam                 # ... and a single coordinate does grow on these rays


def test_issue_table_levels_alive():
    """the issue's fp64 case: a unit direction scaled to norm-tensor 800 from the origin, 128 intervals uniform in disparity from 0.2 to
    1e6, r = 2 / sqrt(12) / 1000.  Highest level whose attenuation is above 0.5: metric against contracted covariance."""
    s = torch.linspace(0, 1, 129, dtype=torch.float64)
    z = (1 / ((1 - s) / 0.2 + s / 1e6))[None, :]
    rays = torch.tensor([[0.0, 0.0, 0.0, 0.6, 0.0, 0.8]], dtype=torch.float64)
    r2 = (2 / 12 ** 0.5 / 1000) ** 2
    alive = {}
    for mode in ("metric", "gaussian"):
        var = G.spec(z, rays, 10, r2, 800.0, mode=mode)[2][0]
        lv = [max([l for l in range(16) if float(torch.exp(-0.5 * 4.0 ** l * var[i].max())) > 0.5], default=None) for i in (100, 120, 127)]
        alive[mode] = lv
    assert alive["metric"][0] == alive["gaussian"][0] and alive["metric"][2] is None
    assert alive["gaussian"][1] > alive["metric"][1] and alive["gaussian"][2] is not None and alive["gaussian"][2] >= alive["gaussian"][0]


# ------------------------------------------------------------------------------------------------ the comparator
def _emulate(z, rays, L, r2, dn, mode="gaussian", fault=None):
    """the kernels' sequence of fp32 operations in torch (CPU: every operation rounds once) -> feat (N,S,6L), mu (N,S,3)"""
    z0, z1 = z[:, :-1, None], z[:, 1:, None]
    r2 = torch.tensor(r2, dtype=torch.float32)
    c512 = torch.tensor(G.FIVE_TWELFTHS_F32, dtype=torch.float32)
    mid, hw = (z1 + z0) / 2, (z1 - z0) / 2
    hw2, mid2 = hw * hw, mid * mid
    t1 = 3 * mid2 + hw2
    mu_t = mid + ((2 * mid) * hw2) / t1
    hw4 = hw2 * hw2
    var_t = hw2 / 3 - (((4 * hw4) * (12 * mid2 - hw2)) / 15) / (t1 * t1)
    var_r = r2 * ((0.25 * mid2 + c512 * hw2) - (4 * hw4) / (15 * t1))
    o, d = rays[:, None, :3], rays[:, None, 3:6]
    x = o + mu_t * d
    dd = d * d
    diag = var_t * dd + var_r * (1 - dd / dn)
    n = ((x[..., 0:1] * x[..., 0:1] + x[..., 1:2] * x[..., 1:2]) + x[..., 2:3] * x[..., 2:3]).sqrt()
    outside = n > 1
    ns = torch.where(outside, n, torch.full_like(n, 2.0))
    t = 1 / ns
    kk = (2 - t) / ns
    mu = torch.where(outside, x * kk, x)
    var = diag
    if mode == "gaussian":
        xh = x * t
        xd = ((xh[..., 0:1] * d[..., 0:1] + xh[..., 1:2] * d[..., 1:2]) + xh[..., 2:3] * d[..., 2:3])
        t2, k2 = t * t, kk * kk
        rad, t4 = xd * t2, t2 * t2
        sq = xh * xh
        jd = kk * (d - xh * xd) + xh * rad
        jj = k2 * (sq[..., [1, 2, 0]] + sq[..., [2, 0, 1]]) + sq * t4
        inv_dn = 1.0
        if fault == "no_axx":                               # J = k I: the radial compression is lost
            jd, jj = kk * d, k2.expand_as(sq)
        elif fault == "diag_only":                          # sum_j J_cj^2 diag_j: the off-diagonal of Sigma is lost
            a = 2 * (1 - ns) / (ns * ns * ns * ns)
            Jm = kk[..., None] * torch.eye(3) + a[..., None] * x[..., :, None] * x[..., None, :]
            pushed = (Jm * Jm * diag[..., None, :]).sum(-1)
        elif fault == "no_dn":                              # Sigma = var_t d d^T + var_r I
            inv_dn = 0.0
        jd2 = jd * jd
        if fault != "diag_only":
            pushed = var_t * jd2 + var_r * (jj - inv_dn * (jd2 / dn))
        var = torch.where(outside, pushed, diag)
        if fault == "ulp_inside":                           # the general expression inside the ball: right to an ulp, not to the bit
            var = torch.where(outside, var, torch.nextafter(diag, torch.full_like(diag, float("inf"))))
    f2 = torch.tensor([2.0 ** l for l in range(L)])[:, None]
    arg = f2 * mu[..., None, :]
    att = torch.exp(-0.5 * ((f2 * f2) * var[..., None, :]))
    feat = torch.cat((torch.sin(arg) * att, torch.cos(arg) * att), dim=-1).reshape(z.shape[0], z.shape[1] - 1, 6 * L)
    return feat, mu


@pytest.mark.parametrize("L,r2", [(10, R2), (4, 2.0 ** -8)])
def test_honest_emulation_is_inside_the_bounds_and_the_faults_are_not(inputs, L, r2):
    """(a comparator sees a fault only where its effect exceeds the rounding: the var_r / dn term is a fraction |d_c|^2 / dn of var_r,
    visible at level 9 with a pixel radius of 2^-10 -- with four levels the radius is 2^-4)"""
    rays, zs, dn = inputs
    seen = {f: 0 for f in ("no_axx", "diag_only", "no_dn", "ulp_inside")}
    for fam, z in zs.items():
        assert G.sphere_gap(z, rays) >= G.SPHERE_GAP
        b = G.kernel_bounds(z, rays, L, r2, dn)
        feat64, mu64, var64 = G.spec(z, rays, L, r2, dn)
        # the exact values the bounds are centred on are the specification's
        assert float((b["feat"].v - feat64).abs().max()) < 1e-9 and float((b["mu"].v - mu64).abs().max()) < 1e-12
        assert float(((b["var"].v - var64).abs() / var64).max()) < 1e-8
        twin = _emulate(z, rays, L, r2, dn, mode="metric")
        G.assert_compare("metric twin " + fam, G.compare(G.kernel_bounds(z, rays, L, r2, dn, mode="metric"), *twin))
        rep = G.compare(b, *_emulate(z, rays, L, r2, dn), twin=twin)
        G.assert_compare("honest emulation " + fam, rep)
        # the bounds are not so wide that the earlier definition would pass as the new one
        if fam != "inside":
            assert G.compare(b, *twin)["feat"] > 1.0, fam
        for fault in seen:
            rep = G.compare(b, *_emulate(z, rays, L, r2, dn, fault=fault), twin=twin)
            bad = rep["inside-bits"] > 0 if fault == "ulp_inside" else rep["feat"] > 1.0
            seen[fault] += int(bad)
            if bad:
                with pytest.raises(AssertionError, match="inside-bits" if fault == "ulp_inside" else "feat"):
                    G.assert_compare(fault, rep)
            if fault == "ulp_inside":
                assert rep["feat"] <= 1.0                   # no tolerance sees one ulp: only the bit comparison does
                assert bad == (fam != "far") or bool(b["inside"].any()) == bad, fam
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["no_axx"] >= 2 and seen["diag_only"] >= 1 and seen["no_dn"] >= 1, seen


def test_bf16_doubling_bounds_contain_the_direct_ones():
    """the recurrences only add roundings: at every element the bf16 path's bound is at least the fp32 path's.  It stays useful: the bf16
    rounding of the store (2^-8) dominates up to level 5; from there the recurrence's own amplification shows -- c' = 1 - 2 s^2 turns an
    error e of s into 4 |s| e, so the worst case grows 4x per level where the angle alone would double: 4^9 . 5 u = 0.08 at level 9."""
    rays, zs, _ = G.make_inputs(5, 3, seed=0)
    dn = float(rays[:, 3:].double().norm().float())
    for z in zs.values():
        a = G.kernel_bounds(z, rays, 10, R2, dn)["feat"]
        b = G.kernel_bounds(z, rays, 10, R2, dn, path="doubling", stored_bf16=True)["feat"]
        assert float((a.v - b.v).abs().max()) < 1e-9
        assert bool((b.e >= a.e).all()) and float(b.e.max()) < 0.25
        assert float(b.e[..., :36].max()) < 2.0 ** -8 + 2e-3 and float(a.e.max()) < 2.0 ** -8


# ------------------------------------------------------------------------------------------------ the Python layer
def test_ipe_cov_argument_errors_need_no_device():
    from nerf_amd import ops, parallel, procedures, training
    from nerf_amd.mip_model import MipNeRF
    assert ops.CONTRACT_GAUSSIAN == 2
    assert ops.ipe_contract(True, 0.01, "contracted") == 2 and ops.ipe_contract(True, True, "contracted") == 2
    assert ops.ipe_contract(True, True, "metric") is True and ops.ipe_contract(False, None, "metric") is False
    assert ops._contract_mode(2) == 2 and ops._contract_mode(True) == 1 and ops._contract_mode(False) == 0 and ops._contract_mode(1) == 1
    net = MipNeRF(10, 4, 256)
    calls = {
        "render_image": lambda **kw: procedures.render_image(None, None, None, 8, 10.0, 2.0, 6.0, **_ipe_kw(kw, "ipe")),
        "_render_rays_by_calls": lambda **kw: procedures._render_rays_by_calls(None, None, None, None, None, None, 8, 2.0, 6.0, False, False,
                                                                                **_ipe_kw(kw, "ipe_radius")),
        "render_image_sharded": lambda **kw: parallel.render_image_sharded(None, None, None, 8, 10.0, 2.0, 6.0, **_ipe_kw(kw, "ipe")),
        "TrainStep": lambda **kw: training.TrainStep(None, None, None, (8, 8), 10.0, 2.0, 6.0, **_ipe_kw(kw, "ipe_radius")),
        "forward_rays": lambda **kw: net.forward_rays(None, None, 4, **_ipe_kw(kw, "ipe_radius")),
    }
    for name, call in calls.items():
        for kw in (dict(ipe=0.01, contract=False, ipe_cov="contracted"), dict(ipe=None, contract=True, ipe_cov="contracted"),
                   dict(ipe=0.01, contract=True, ipe_cov="Contracted"), dict(ipe=None, contract=False, ipe_cov="gaussian")):
            with pytest.raises(ValueError, match="ipe_cov"):
                call(**kw)
    for fn in (procedures.render_image, procedures._render_rays_by_calls, parallel.render_image_sharded, training.TrainStep.__init__,
               MipNeRF.forward_rays):
        p = inspect.signature(fn).parameters["ipe_cov"]
        assert p.default == "metric" and (p.kind is inspect.Parameter.KEYWORD_ONLY or fn is procedures._render_rays_by_calls), fn
    assert inspect.signature(procedures._render_rays_by_calls).parameters["ipe_cov"].kind is inspect.Parameter.KEYWORD_ONLY


def _ipe_kw(kw, name):
    kw = dict(kw)
    ipe = kw.pop("ipe")
    if name == "ipe":
        kw["ipe"] = False if ipe is None else ipe
    else:
        kw["ipe_radius"] = ipe
    return kw


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_symbol_is_declared_bound_and_the_abi_number_stays():
    from nerf_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    assert "#define NERF_AMD_CONTRACT_GAUSSIAN 2" in header and _lib.CONTRACT_GAUSSIAN == 2
    assert "int nerf_amd_ipe_feature_gaussian(const float* z, const float* rays, int64_t N, int S, int L, float r, const float* dir_norm," in header
    name = "nerf_amd_ipe_feature_gaussian"
    assert name in _lib.ADDED_AFTER_125 and hasattr(_lib.lib, name)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES["nerf_amd_ipe_feature_contracted"] and len(_lib.SIGNATURES[name][1]) == 11
    fn = getattr(_lib.lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert _lib.lib.nerf_amd_version() == 125 and _lib.EXPECTED_VERSION == 125
    launchers = open(os.path.join(ROOT, "nerf_amd", "csrc", "launchers.h")).read()
    assert launchers.count("int sk_ipe_feature(") == 1              # one launcher serves the three entry points: `contract` is its argument
    assert header.count(name + "(") == 1 and sum(1 for k in _lib.SIGNATURES if k == name) == 1
    # N = 0: every size check passes and nothing is launched; a bad L is refused like its twins'
    assert fn(None, None, 0, 4, 10, 0.01, None, None, None, None, None) == 0
    assert fn(None, None, 0, 4, 16, 0.01, None, None, None, None, None) == -1
    assert fn(None, None, 4, 4, 10, 0.01, None, None, None, None, None) == -1 and b"NULL" in _lib.lib.nerf_amd_last_error()


def test_abi_refuses_the_gaussian_mode_where_it_has_no_meaning():
    """on empty descriptors (M = 0, N = 0): every check runs, nothing is launched"""
    from nerf_amd import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)

    def points(contract):
        s = _lib.Samples()
        s.mode, s.M, s.pts_stride, s.contract = 0, 0, 6, contract
        return s

    def frusta(contract):
        s = _lib.Samples()
        s.mode, s.S, s.M, s.rays, s.z, s.z_stride, s.contract = 1, 4, 0, ptr, ptr, 5, contract
        s.ipe, s.ipe_radius, s.ipe_dir_norm = 1, 0.01, ptr
        return s

    for fn, extra in ((lib.nerf_amd_mip_forward, (ptr, None)), (lib.nerf_amd_mip_forward_train, (ptr, ptr, None))):
        for c in (0, 1):
            assert fn(ptr, _lib.F32, C.byref(points(c)), *extra) == 0, (fn, c)
        for c in (0, 1, 2):
            assert fn(ptr, _lib.F32, C.byref(frusta(c)), *extra) == 0, (fn, c)
        assert fn(ptr, _lib.F32, C.byref(points(2)), *extra) == -1 and b"integrated PE" in lib.nerf_amd_last_error()
        for c in (3, -1, 256):
            assert fn(ptr, _lib.F32, C.byref(points(c)), *extra) == -1 and b"contract" in lib.nerf_amd_last_error(), c
            assert fn(ptr, _lib.F32, C.byref(frusta(c)), *extra) == -1, c
    # the proposal and Ref-NeRF kernels encode points: 2 is read as 1; other values are refused there too
    s3 = points(2)
    s3.pts_stride = 3
    assert lib.nerf_amd_proposal_forward(ptr, _lib.F32, C.byref(s3), ptr, None) == 0
    assert lib.nerf_amd_ref_forward(ptr, _lib.F32, C.byref(points(2)), 0, ptr, ptr, None) == 0
    s3.contract = 3
    assert lib.nerf_amd_proposal_forward(ptr, _lib.F32, C.byref(s3), ptr, None) == -1
    assert lib.nerf_amd_ref_forward(ptr, _lib.F32, C.byref(points(7)), 0, ptr, ptr, None) == -1
    # the render entry points carry the value in `camera`
    cam = _lib.Samples()

    def render(contract, ipe):
        cam.contract, cam.ipe, cam.ipe_radius = contract, ipe, 0.01
        # packed_prop packed_mip precision rays camera ray_offset z_base u_strat u_inv N n_fine near far white_bkg rgb depth weights workspace stream
        return lib.nerf_amd_render_rays(ptr, ptr, _lib.F32, ptr, C.byref(cam), 0, ptr, None, None, 0, 64, 2.0, 6.0, 1, ptr, None, None, ptr, None)

    assert render(0, 0) == 0 and render(1, 0) == 0 and render(1, 1) == 0 and render(2, 1) == 0
    assert render(2, 0) == -1 and b"integrated PE" in lib.nerf_amd_last_error()
    assert render(3, 1) == -1 and render(-2, 0) == -1
