"""The empty-ray skip on the GPU (nerf_amd_ray_alive, nerf_amd_gather_rows, nerf_amd_render with skip_min_optical_depth,
render_image(skip_empty=...)).  The stage is checked against the fp64 specification of tests/skip_empty_ref.py, exactly: the thresholds
leave no ray undecidable (asserted).  The pipelines are checked against their own dense render, bit for bit: an alive ray is the dense
ray, a dead ray is ops.composite of an all-zero row on its own depth row."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import skip_empty_ref as R
import weights as W
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
SEED = 4711
TAU = 0.5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")
    yield
    nerf_amd.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ the stand-alone stage
GUARD = 64                                                                 # elements in front of and behind every output, which must keep their fill


def _guarded(n, dtype, fill):
    """a buffer of GUARD + n + GUARD elements whose every BYTE is `fill` -> (whole, the n elements in the middle)"""
    whole = torch.empty(((2 * GUARD + n) * torch.empty((), dtype=dtype).element_size(),), dtype=torch.uint8, device="cuda").fill_(fill).view(dtype)
    return whole, whole[GUARD: GUARD + n]


def _run_stage(density, z, dirs, d_min, fill, z_pad=0, d_pad=0):
    """nerf_amd_ray_alive through ctypes on guarded, pre-filled outputs and padded input rows -> (row_of_ray, ray_of_row (N,), count), numpy;
    asserts that nothing outside the outputs was written"""
    from nerf_amd import _lib
    N, C = density.shape
    zt = torch.full((N, C + z_pad), float("nan"), device="cuda")
    zt[:, :C] = torch.from_numpy(z).cuda()
    dt = torch.full((N, 3 + d_pad), float("nan"), device="cuda")
    dt[:, :3] = torch.from_numpy(dirs).cuda()
    den = torch.from_numpy(density).cuda()
    row_w, row = _guarded(N, torch.int32, fill)
    ray_w, ray = _guarded(N, torch.int64, fill)
    cnt_w, cnt = _guarded(1, torch.int64, fill)
    ws = torch.empty(max(int(_lib.lib.nerf_amd_ray_alive_workspace_bytes(N)), 1), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.nerf_amd_ray_alive(den.data_ptr(), zt.data_ptr(), C + z_pad, dt.data_ptr(), 3 + d_pad, N, C, float(d_min), row.data_ptr(), ray.data_ptr(),
                                           cnt.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "nerf_amd_ray_alive")
    torch.cuda.synchronize()
    for whole, n in ((row_w, N), (ray_w, N), (cnt_w, 1)):
        b = whole.view(torch.uint8).view(2 * GUARD + n, -1)
        assert bool((b[:GUARD] == fill).all()) and bool((b[GUARD + n:] == fill).all()), "a write outside an output"
    return row.cpu().numpy(), ray.cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("C", R.GPU_C)
@pytest.mark.parametrize("N", R.GPU_N)
def test_stage_equals_the_specification(N, C):
    """flags and both tables, exactly; N' = 0 (an infinite threshold on inputs without a NaN), 1 (the NaN row alone survives it), N (a
    negative threshold) and in between; padded strides; both fills; two runs"""
    density, z, dirs = R.make_inputs(N, C, 0)
    plain = R.make_inputs(N, C, 1, special=False)
    seen = set()
    for (den, zz, dd), d_min, pads in (((density, z, dirs), R.d_min_of_tau(TAU), (0, 0)), ((density, z, dirs), R.d_min_of_tau(1e-3), (5, 3)),
                                       ((density, z, dirs), -1.0, (1, 0)), ((density, z, dirs), np.inf, (0, 1)), (plain, np.inf, (3, 3))):
        want = R.spec(den, zz, dd, d_min)
        assert int(R.undecidable(want["D"], d_min).sum()) == 0
        runs = [_run_stage(den, zz, dd, d_min, fill, *pads) for fill in (0x00, 0xFF, 0xFF)]
        n = want["n_alive"]
        seen.add(n)
        for fill, (row, ray, count) in zip((0x00, 0xFF, 0xFF), runs):
            assert count == n, (d_min, count, n)
            assert np.array_equal(row, want["row_of_ray"]), d_min
            assert np.array_equal(ray[:n], want["ray_of_row"]), d_min
            tail = np.frombuffer(ray[n:].tobytes(), np.uint8)
            assert bool((tail == fill).all()), "ray_of_row is written beyond N'"
        assert all(np.array_equal(a, b) for a, b in zip(runs[1][:2], runs[2][:2]))                   # the same bits twice
    assert {0, N} <= seen and (N < 63 or (1 in seen and any(0 < v < N for v in seen))), seen


def test_gather_rows_and_the_python_op():
    from nerf_amd import ops
    density, z, dirs = R.make_inputs(1000, 65, 2)
    want = R.spec(density, z, dirs, R.d_min_of_tau(TAU))
    rays = torch.cat((torch.zeros(1000, 3), torch.from_numpy(dirs)), 1).cuda()
    zt = torch.full((1000, 70), -1.0, device="cuda")
    zt[:, :65] = torch.from_numpy(z).cuda()
    for d in (torch.from_numpy(dirs).cuda(), rays):                        # (N,3) directions, and the (N,6) ray table read in place
        row, ray, n = ops.ray_alive(torch.from_numpy(density).cuda(), zt[:, :65], d, tau=TAU)
        assert n == want["n_alive"] and row.dtype == torch.int32 and ray.dtype == torch.int64 and ray.shape == (n,)
        assert np.array_equal(row.cpu().numpy(), want["row_of_ray"]) and np.array_equal(ray.cpu().numpy(), want["ray_of_row"])
    row2, ray2, n2 = ops.ray_alive(torch.from_numpy(density).cuda(), zt[:, :65], rays, min_optical_depth=R.d_min_of_tau(TAU))
    assert n2 == n and torch.equal(row2, row)
    got = ops.gather_rows(zt[:, :65], ray)                                 # a strided source
    assert got.shape == (n, 65) and torch.equal(got, zt[:, :65][ray])
    assert torch.equal(ops.gather_rows(rays, ray), rays[ray])
    assert ops.gather_rows(rays, ray[:0]).shape == (0, 6)
    e = ops.ray_alive(torch.zeros(0, 8).cuda(), torch.zeros(0, 8).cuda(), torch.zeros(0, 3).cuda(), tau=TAU)
    assert e[2] == 0 and e[0].shape == (0,) and e[1].shape == (0,)


# ------------------------------------------------------------------------------------------------ the pipelines
SIDE = 45                                                                  # 2 025 rays: the last tile of every kernel is ragged
QS = (0.1, 0.5)
SPACINGS = {"linear": (2.0, 6.0), "disparity": (0.2, 1000.0)}
# every covered run: fp32 and bf16, linear with explicit uniforms and with Philox, disparity, two rounds with prop_pnum 3 and 64, Ref-NeRF with
# normal_img, the integrated PE with the contracted covariance, white_bkg on and off, n_fine 16 and 128 -- all with quantiles, opacity and
# fine_depths on
CONFIGS = {
    "linear-fp32-uniforms-nf128-white": dict(route="plain", spacing="linear", prec="fp32", nf=128, white=True, uniforms=True),
    "linear-bf16-philox-nf16-black": dict(route="plain", spacing="linear", prec="bf16", nf=16, white=False),
    "disparity-fp32-nf16-white": dict(route="warped", spacing="disparity", prec="fp32", nf=16, white=True, contract=True),
    "disparity-bf16-nf128-black": dict(route="warped", spacing="disparity", prec="bf16", nf=128, white=False, contract=True),
    "rounds3-linear-fp32-nf16": dict(route="rounds", spacing="linear", prec="fp32", nf=16, white=True, P=3),
    "rounds64-disparity-bf16-nf128": dict(route="rounds", spacing="disparity", prec="bf16", nf=128, white=False, P=64, contract=True),
    "ref-fp32-nf16-normals": dict(route="ref", spacing="linear", prec="fp32", nf=16, white=True),
    "ref-bf16-nf128-normals": dict(route="ref", spacing="linear", prec="bf16", nf=128, white=False),
    "ipe-contracted-fp32-nf128": dict(route="plain", spacing="linear", prec="fp32", nf=128, white=True, contract=True, ipe=True),
}
OUTPUTS = ("rgb", "depth", "weights", "opacity", "depth_q", "fine_depths", "normal_img")


def _camera(side=SIDE):
    return O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda(), O.fov2focal(0.6911112070083618, (side, side))


@functools.lru_cache(maxsize=None)
def _rays():
    from nerf_amd import ops, utils
    pose, focal = _camera()
    fx, fy = utils._focal_xy(focal)
    return ops.generate_rays(pose, SIDE, SIDE, fx, fy, pose.device)


def _precision(name):
    import nerf_amd
    from nerf_amd import ops
    nerf_amd.set_precision(name)
    return ops.BF16 if name == "bf16" else ops.F32


def _family(c):
    return (c["spacing"], bool(c.get("contract")))


def _coarse(c, prop, rays, off=0):
    """the coarse draw and the first proposal pass, call by call -> (u1, z (N,64) metric, s_c | None, density (N,64))"""
    from nerf_amd import ops
    near, far = SPACINGS[c["spacing"]]
    n = rays.shape[0]
    if c.get("uniforms"):
        u1 = torch.rand((n, 64), device="cuda", generator=torch.Generator("cuda").manual_seed(SEED))
    else:
        u1 = ops.philox_stream((n, 64), SEED, off, strat=True, device=rays.device)
    s_c = None
    if c["spacing"] == "disparity":
        s_c, z, pts = ops.warped_stratified(rays, u1, near, far)
    else:
        z, pts = ops.stratified_points(rays, torch.linspace(near, far, 64).cuda(), u1, (far - near) / c["nf"])
    return u1, z, s_c, (prop.forward(pts, contract=True) if c.get("contract") else prop.forward(pts))


@functools.lru_cache(maxsize=None)
def _nets(family, kind):
    """(prop, mip, ref) on the synthetic weights; kind "half": the proposal head's bias is shifted by the median of the network's own coarse
    density on the test's rays (about half the densities are then negative); "full": untouched (every density is positive: no ray is empty);
    "empty": shifted below the smallest density (every ray is empty)"""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.ref_model import RefNeRF
    prop, mip, ref = ProposalNetwork(10, 256), MipNeRF(10, 4, 256), RefNeRF(10, 4)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small"))
    ref.load_state_dict(W.ref_state("small"))
    prop, mip, ref = prop.cuda().eval(), mip.cuda().eval(), ref.cuda().eval()
    if kind != "full":
        _precision("fp32")
        with torch.no_grad():
            den = _coarse(dict(spacing=family[0], contract=family[1], nf=128), prop, _rays())[3]
            prop.layers[8].bias -= float(den.median()) if kind == "half" else float(den.max()) + 1.0
        ops.parameters_changed()
    return prop, mip, ref


def _histogram(name, kind="half", off=0, rays=None):
    """the histogram the fine depths are drawn from, through the call-by-call ops -> (density, z) numpy"""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import inverseSample
    c = CONFIGS[name]
    rays = _rays() if rays is None else rays
    prop = _nets(_family(c), kind)[0]
    near, far = SPACINGS[c["spacing"]]
    _precision(c["prec"])
    with torch.no_grad():
        _, z, s_c, den = _coarse(c, prop, rays, off)
        if c["route"] == "rounds":
            P = c["P"]
            w = maxBlurFilter(ProposalNetwork.get_weights(den, z, rays[:, 3:]), 0.01)
            u_mid = ops.philox_stream((rays.shape[0], P + c["nf"] + 1), SEED, off, device=rays.device)[:, :P].contiguous()
            if s_c is not None:
                s_mid, _ = inverseSample(w, s_c, P, sort=True, u=u_mid)
                z, pts = ops.warp_depths(s_mid, near, far, rays)
            else:
                z, _ = inverseSample(w, z, P, sort=True, u=u_mid)
                pts = NeRF.length2pts(rays, z)[..., :3].contiguous()
            den = prop.forward(pts, contract=True) if c.get("contract") else prop.forward(pts)
    return den.cpu().numpy(), z.cpu().numpy()


def _ipe_kw(c, rays_all):
    from nerf_amd import ops, utils
    if not c.get("ipe"):
        return dict(contract=bool(c.get("contract")))
    return dict(contract=ops.ipe_contract(True, True, "contracted"), ipe_radius=2.0 / (12.0 ** 0.5) / utils._focal_xy(_camera()[1])[0],
                ipe_dir_norm=ops.dirs_norm(rays_all))


def _render(name, kind="half", off=0, rays=None, **skip):
    """one fused render call of a configuration -> dict of its outputs (and, with the skip on, row_of_ray and n_alive)"""
    from nerf_amd import ops
    c = CONFIGS[name]
    all_rays = _rays()
    rays = all_rays if rays is None else rays
    prop, mip, ref = _nets(_family(c), kind)
    near, far = SPACINGS[c["spacing"]]
    prec = _precision(c["prec"])
    z_base = torch.linspace(near, far, 64).cuda()
    n, nf = rays.shape[0], c["nf"]
    common = dict(quantiles=QS, want_opacity=True, want_fine_depths=True, **skip)
    u1 = u2 = None
    if c.get("uniforms"):
        u1 = torch.rand((n, 64), device="cuda", generator=torch.Generator("cuda").manual_seed(SEED))
        u2 = torch.rand((n, nf + 1), device="cuda", generator=torch.Generator("cuda").manual_seed(SEED + 1))
    seed = None if c.get("uniforms") else SEED
    with torch.no_grad():
        if c["route"] == "ref":
            out = ops.render_rays_ref(prop.packed(prec), ref.packed(prec), prec, rays, z_base, u1, u2, nf, near, far, c["white"], cam_dir=_camera()[0][:, -2].contiguous(),
                                      flags=ref.kernel_flags, seed=seed, rng_ray_offset=off, **common)
            res = dict(rgb=out[0], depth=out[1], normal_img=out[2], weights=out[-1]["weights"])
        else:
            packed = (prop.packed(prec), mip.packed(prec, wide=bool(c.get("ipe"))), prec, rays)
            kw = dict(want_weights=True, seed=seed, rng_ray_offset=off, **_ipe_kw(c, all_rays), **common)
            if c["route"] == "rounds":
                out = ops._render_rays_rounds(*packed, z_base, nf, near, far, c["white"], prop_pnum=c["P"], spacing=c["spacing"], **kw)
            elif c["route"] == "warped":
                out = ops.render_rays_warped(*packed, u1, u2, nf, near, far, c["white"], **kw)
            else:
                out = ops.render_rays(*packed, z_base, u1, u2, nf, near, far, c["white"], **kw)
            res = dict(rgb=out[0], depth=out[1], weights=out[2], normal_img=None)
    res.update({k: out[-1][k] for k in ("opacity", "depth_q", "fine_depths", "row_of_ray", "n_alive") if k in out[-1]})
    return res


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(the dense render, the render with the skip on) of a configuration, on the half-empty weights; rendered once, never written to"""
    return _render(name), _render(name, skip_tau=TAU)


def _dead_reference(name, out, dead):
    """what the dense kernels make of all-zero fine-network rows on the dead rays' own depth rows -> dict like _render's"""
    from nerf_amd import ops
    c = CONFIGS[name]
    near, far = SPACINGS[c["spacing"]]
    warped = c["spacing"] == "disparity"
    rays = _rays()[dead].contiguous()
    z = out["fine_depths"][dead].contiguous()
    m, S = rays.shape[0], out["weights"].shape[1]
    zero = torch.zeros((m, S, 4), device="cuda")
    nf_range = (0.0, 1.0) if warped else (near, far)
    if c["route"] == "ref":
        rgb, w, depth, nimg = ops.composite(zero, z, rays, True, c["white"], ops.ACT_SOFTPLUS, (near, far), normal=torch.zeros((m, S, 3), device="cuda"),
                                            cam_dir=_camera()[0][:, -2].contiguous(), sigma_shift=0.5)
    else:
        rgb, w, depth, nimg = ops.composite(zero, z, rays, True, c["white"], ops.ACT_RELU, nf_range)
    dq, op = ops.ray_depth_stats(w, z, rays, quantiles=QS, near=nf_range[0], far=nf_range[1])
    if warped:
        depth = ops.warp_depths(depth.reshape(m, 1), near, far, inverse=True)[0].reshape(-1)
        dq = ops.warp_depths(dq, near, far, inverse=True)[0]
    return dict(rgb=rgb, depth=depth, weights=w, opacity=op, depth_q=dq, fine_depths=z, normal_img=nimg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_mask_is_the_specification_on_the_pipelines_own_histogram(name):
    dense, skip = _pair(name)
    density, z = _histogram(name)
    d_min = R.d_min_of_tau(TAU)
    want = R.spec(density, z, _rays()[:, 3:].cpu().numpy(), d_min)
    assert int(R.undecidable(want["D"], d_min).sum()) == 0
    n = _rays().shape[0]
    dead_fraction = 1.0 - skip["n_alive"] / n
    print("%s: %d of %d rays alive (dead fraction %.3f)" % (name, skip["n_alive"], n, dead_fraction))
    assert 0.25 <= dead_fraction <= 0.75
    assert skip["n_alive"] == want["n_alive"] and np.array_equal(skip["row_of_ray"].cpu().numpy(), want["row_of_ray"])
    assert "row_of_ray" not in dense and "n_alive" not in dense


@pytest.mark.parametrize("name", list(CONFIGS))
def test_alive_rays_are_the_dense_render_and_dead_rays_composite_zero_rows(name):
    c = CONFIGS[name]
    dense, skip = _pair(name)
    alive = skip["row_of_ray"] >= 0
    dead = (~alive).nonzero().reshape(-1)
    assert 0 < dead.numel() < alive.numel()
    want = _dead_reference(name, skip, dead)
    for k in OUTPUTS:
        if dense[k] is None:
            assert skip[k] is None and k == "normal_img" and c["route"] != "ref"
            continue
        assert skip[k].shape == dense[k].shape and bool(torch.isfinite(skip[k]).all()), k
        assert torch.equal(skip[k][alive], dense[k][alive]), "%s: an alive ray differs from the dense render in %s" % (name, k)
        assert torch.equal(skip[k][dead], want[k]), "%s: a dead ray is not the composite of zero rows in %s" % (name, k)
    assert torch.equal(skip["fine_depths"], dense["fine_depths"])         # the depth rows are the dense call's on every ray
    assert float(dense["rgb"][alive].std()) > 0.0                          # not a constant image (Ref-NeRF's synthetic weights: std 7e-4)
    if c["route"] != "ref":                                                # zero density: the background, nothing accumulated, the far edge
        near, far = SPACINGS[c["spacing"]]
        assert bool((skip["weights"][dead] == 0).all()) and bool((skip["opacity"][dead] == 0).all())
        assert bool((skip["rgb"][dead] == (1.0 if c["white"] else 0.0)).all())
        assert not torch.equal(dense["rgb"][dead], skip["rgb"][dead])      # (the approximation is visible on these weights: the skip did something)


@pytest.mark.parametrize("name", ["linear-bf16-philox-nf16-black", "rounds64-disparity-bf16-nf128", "ref-fp32-nf16-normals", "ipe-contracted-fp32-nf128"])
def test_all_alive_is_the_dense_render_and_all_dead_is_the_background(name):
    c = CONFIGS[name]
    n = _rays().shape[0]
    dense, skip = _render(name, "full"), _render(name, "full", skip_tau=1e-3)
    assert skip["n_alive"] == n and torch.equal(skip["row_of_ray"], torch.arange(n, dtype=torch.int32, device="cuda"))
    for k in OUTPUTS:
        assert (dense[k] is None and skip[k] is None) or torch.equal(dense[k], skip[k]), k
    empty = _render(name, "empty", skip_tau=TAU)                          # no ray alive: the code's n_alive == 0 path launches no fine network
    assert empty["n_alive"] == 0 and bool((empty["row_of_ray"] == -1).all())
    want = _dead_reference(name, empty, torch.arange(n, device="cuda"))
    for k in OUTPUTS:
        assert (want[k] is None and empty[k] is None) or torch.equal(empty[k], want[k]), k
    if c["route"] != "ref":
        assert bool((empty["rgb"] == (1.0 if c["white"] else 0.0)).all()) and bool((empty["opacity"] == 0).all())


def _image_kw(name):
    c = CONFIGS[name]
    near, far = SPACINGS[c["spacing"]]
    prop, mip, ref = _nets(_family(c), "half")
    kw = dict(white_bkg=c["white"], render_depth=True, render_normal=c["route"] == "ref", contract=bool(c.get("contract")), ipe=bool(c.get("ipe")), seed=SEED,
              spacing=c["spacing"], depth_quantiles=QS, render_opacity=True)
    if c["route"] == "rounds":
        kw.update(prop_rounds=2, prop_pnum=c["P"])
    if c.get("ipe"):
        kw.update(ipe_cov="contracted")
    return (ref if c["route"] == "ref" else mip, prop, _camera()[0], SIDE, _camera()[1], near, far, c["nf"]), kw


SHARDED = ["linear-bf16-philox-nf16-black", "disparity-fp32-nf16-white", "rounds64-disparity-bf16-nf128", "ref-fp32-nf16-normals", "ipe-contracted-fp32-nf128"]


@pytest.mark.parametrize("name", SHARDED)
def test_three_shards_and_the_call_by_call_route_give_the_bits_of_one_fused_call(name, monkeypatch):
    from nerf_amd import procedures
    c = CONFIGS[name]
    _precision(c["prec"])
    args, kw = _image_kw(name)
    n = SIDE * SIDE
    keys = ("rgb_rays", "depth_rays", "depth_q_rays", "opacity_rays", "alive_rays") + (("normal_rays",) if c["route"] == "ref" else ())
    with torch.no_grad():
        one = procedures.render_image(*args, **kw, skip_empty=TAU, _shard=(0, n))
        parts = [procedures.render_image(*args, **kw, skip_empty=TAU, _shard=cut) for cut in ((0, 700), (700, 1400), (1400, n))]
        monkeypatch.setattr(procedures, "_render_route", lambda *a: "calls")
        calls = procedures.render_image(*args, **kw, skip_empty=TAU, _shard=(0, n))
    fused = _pair(name)[1]
    assert torch.equal(one["rgb_rays"], fused["rgb"]) and torch.equal(one["alive_rays"], fused["row_of_ray"] >= 0)      # (an un-tiled image: raster order)
    assert 0 < int(one["alive_rays"].sum()) < n and one["alive_rays"].dtype == torch.bool
    for k in keys:
        assert torch.equal(torch.cat([p[k] for p in parts]), one[k]), "%s: three shards differ from one call in %s" % (name, k)
        assert torch.equal(calls[k], one[k]), "%s: the call-by-call route differs from the fused one in %s" % (name, k)


def test_render_image_keys_shapes_and_the_fraction():
    from nerf_amd import procedures
    name = "linear-bf16-philox-nf16-black"
    _precision("bf16")
    prop, mip, _ = _nets(_family(CONFIGS[name]), "half")
    pose, focal = _camera(50)
    args = (mip, prop, pose, (50, 40), focal, 2.0, 6.0, 16)
    with torch.no_grad():
        dense = procedures.render_image(*args, render_depth=True, seed=SEED)
        again = procedures.render_image(*args, render_depth=True, seed=SEED, skip_empty=None)
        skip = procedures.render_image(*args, render_depth=True, seed=SEED, skip_empty=TAU)
    assert set(dense) == set(again) == {"rgb", "depth_img"} and all(torch.equal(dense[k], again[k]) for k in dense)       # the keyword left out: the dict of today
    assert set(skip) == {"rgb", "depth_img", "alive_img", "alive_fraction"}
    assert skip["rgb"].shape == (3, 50, 40) and skip["depth_img"].shape == (3, 50, 40)
    assert skip["alive_img"].shape == (50, 40) and skip["alive_img"].dtype == torch.bool and isinstance(skip["alive_fraction"], float)
    assert skip["alive_fraction"] == float(skip["alive_img"].double().mean()) and 0.0 < skip["alive_fraction"] < 1.0
    a = skip["alive_img"]
    assert torch.equal(skip["rgb"][:, a], dense["rgb"][:, a]) and torch.equal(skip["depth_img"][:, a], dense["depth_img"][:, a])
    assert not torch.equal(skip["rgb"], dense["rgb"])


def test_the_skip_is_refused_on_a_capturing_stream():
    from nerf_amd import _lib, ops
    name = "linear-bf16-philox-nf16-black"
    _render(name, skip_tau=TAU)                                            # (warm: the weights are packed before the capture)
    prop, mip, _ = _nets(_family(CONFIGS[name]), "half")
    prec = _precision("bf16")
    args = (prop.packed(prec), mip.packed(prec), prec, _rays(), torch.linspace(2.0, 6.0, 64).cuda(), None, None, 16, 2.0, 6.0, False)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    caught, keep = None, torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):                             # refused on the host before any launch: the graph holds the one add
        keep.add_(1.0)
        try:
            ops.render_rays(*args, seed=SEED, skip_tau=TAU)
        except _lib.NerfAmdError as e:
            caught = str(e)
    torch.cuda.synchronize()
    assert caught is not None and "(-2)" in caught and "captur" in caught
    with torch.no_grad():                                                  # and the same call outside a capture still renders
        assert ops.render_rays(*args, seed=SEED, skip_tau=TAU)[-1]["n_alive"] == _pair(name)[1]["n_alive"]
