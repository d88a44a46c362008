"""The integrated PE with the WHOLE frustum Gaussian contracted (nerf_amd_samples.contract = NERF_AMD_CONTRACT_GAUSSIAN, `ipe_cov="contracted"`)
on the GPU, at every layer it reaches.  tests/ipe_gaussian_ref.py holds the fp64 specification and the derivation of every bound;
tests/test_ipe_gaussian_host.py shows on the CPU that the comparator passes an honest fp32 emulation and reports four planted faults.

  1. the stand-alone encoder (nerf_amd_ipe_feature_gaussian): feat and mu against fp64 within the derived bounds;
  2. the fused training forward, fp32 and bf16: the dumped encoding slot against fp64 within the derived bounds, and the layer
     comparators of forward_ref on the same dump;
  3. the render kernel and the fp8-dump forward equal the training forward bit for bit;
  4. inside the unit ball the mode is contract = 1, bit for bit;
  5. far rays: other outputs, the same mean, and the attenuation only grows -- element-wise on rays through the origin, as the
     product over the three coordinates on every ray (ipe_gaussian_ref: WHAT HOLDS BETWEEN THE TWO MODES; the issue's element-wise
     statement for every ray is not a property of J Sigma J^T: it fails in the fp64 specification on about 1 % of the elements of
     these inputs, tests/test_ipe_gaussian_host.py asserts that too);
  6. render_image through every route, the layer-by-layer route against the oracle's network on the specification's features, shards;
  7. TrainStep: eager == replayed, inside-ball gradients == the metric mode's, far losses finite and different.

Inputs everywhere (ipe_gaussian_ref.make_inputs): origins in [-0.5, 0.5]^3, unnormalised randn directions with |d|^2 < dn, three depth
families per ray set -- inside the ball, straddling it, geometric out to 1e6 -- and no metric mean within 1e-4 of the unit sphere."""
import ctypes
import math

import pytest
import torch

import forward_ref as F
import ipe_gaussian_ref as G
import test_gpu_forward_layers as TL
import weights as W
from conftest import gate, max_abs
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

RADIUS = 2.0 / 12.0 ** 0.5 / 55.0
R2 = float(torch.tensor(RADIUS * RADIUS, dtype=torch.float64).float())           # the fp32 value the entry points hand the kernels
SEED = 20221


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import ops
    from nerf_amd import _lib

    class NS:
        pass
    ns = NS()
    ns.pkg, ns.ops, ns.lib = nerf_amd, ops, _lib.lib
    ns.ids = {"prop": _lib.NET_PROPOSAL, "mip": _lib.NET_MIP, "prop128": _lib.NET_PROPOSAL_128, "mip128": _lib.NET_MIP_128}
    n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
    assert ns.lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
    ns.n_cu = int(n_cu.value)
    ns.nets = {}
    nerf_amd.set_precision("fp32")
    yield ns
    nerf_amd.set_precision("fp32")


_INPUTS = {}


def _inputs(N, S, need_gap=True):
    """-> (rays, {family: z}, rays on the device, {family: z on the device}, dn on the device, dn): computed once per shape, never written"""
    key = (N, S, need_gap)
    if key not in _INPUTS:
        from nerf_amd import ops
        rays, zs, _ = G.make_inputs(N, S, seed=100 * N + S, need_gap=need_gap)
        d2 = (rays[:, 3:].double() ** 2).sum(-1)
        rd = rays.cuda()
        dn_dev = ops.dirs_norm(rd)
        dn = float(dn_dev.cpu())
        assert bool((d2 < dn).all())                                                # |d|^2 < dn: Sigma is positive definite
        if need_gap:
            assert min(G.sphere_gap(z, rays) for z in zs.values()) >= G.SPHERE_GAP
        _INPUTS[key] = (rays, zs, rd, {k: z.cuda() for k, z in zs.items()}, dn_dev, dn)
    return _INPUTS[key]


def _emit(prefix, worst):
    failed = []
    for k in sorted(worst):
        try:
            gate("%s %s %s" % (prefix, k, "differing bits" if k == "inside-bits" else "max(err/tol)"), worst[k], 0.0 if k == "inside-bits" else 1.0)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def _merge(worst, rep):
    for k, v in rep.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _same_bits(a, b, what):
    a, b = a.reshape(-1).float().view(torch.int32), b.reshape(-1).float().view(torch.int32)
    assert a.shape == b.shape and torch.equal(a, b), "%s: %d values differ" % (what, int((a != b).sum()) if a.shape == b.shape else -1)


# ------------------------------------------------------------------------------------------------ 1: the stand-alone encoder
@pytest.mark.parametrize("L", [10, 4])
@pytest.mark.parametrize("N,S", [(1, 1), (5, 3), (33, 32)])
def test_encoder_against_the_fp64_specification(A, N, S, L):
    """(33, 32): 1056 samples, not a multiple of the encoder's 64-sample tile, more than one workgroup"""
    rays, zs, rd, zd, dn_dev, dn = _inputs(N, S)
    worst = {}
    for fam in G.FAMILIES:
        feat, mu, mu_t = A.ops.ipe_feature(zd[fam], rd, L, RADIUS, dn_dev, contract=A.ops.CONTRACT_GAUSSIAN)
        twin = A.ops.ipe_feature(zd[fam], rd, L, RADIUS, dn_dev, contract=True)
        _same_bits(mu_t, twin[2], "mu_t")
        rep = G.compare(G.kernel_bounds(zs[fam], rays, L, R2, dn), feat.cpu(), mu.cpu(), twin=(twin[0].cpu(), twin[1].cpu()))
        print("encoder %dx%d L=%d %s: %s" % (N, S, L, fam, rep))
        _merge(worst, rep)
    _emit("ipe-gaussian encoder %dx%d L=%d" % (N, S, L), worst)


# ------------------------------------------------------------------------------------------------ 2: the fused training forward
def _descriptor(A, rd, S, z, dn_dev, contract):
    return A.ops.samples_rays(rd, S, z=z, contract=contract, ipe_radius=RADIUS, ipe_dir_norm=dn_dev)


def _train_forward(A, net, prec, rd, S, z, dn_dev, contract, fmt=None):
    P = A.ops.BF16_F8 if fmt == "fp8" else TL._code(A, prec)
    return A.ops.mip_forward_train_samples(net.packed(A, prec), P, _descriptor(A, rd, S, z, dn_dev, contract), (rd.shape[0], S), "cuda")


def _encoding_slot(A, net, prec, M, dump):
    """-> (mu (M,3), feat (M,60)) of the dumped encoding slot in the reference's column order, as float32 on the CPU"""
    _, enc, _ = TL._read(A, net, prec, M, dump)
    ex, _ = F.encodings("mip", enc)
    ex = ex.float().cpu()
    return ex[:, :3], ex[:, 3:]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_forward_dump_against_the_fp64_specification(A, prec):
    """33 rays x 32 samples = 1056: neither forward tile divides it.  The encoding slot within the derived bounds (bf16: the angle-doubling
    and att^4 recurrences and the rounding of the stored element are in them), then every layer of forward_ref.check_forward on the dump.
    Measured on an MI355X, worst max(err / tol) over the three depth families: fp32 feat 0.828, mu 0.899; bf16 feat 0.993, mu 0.978
    (round-to-nearest attains the bf16 half-ulp term); forward_ref.check_forward on the same dumps: 0.075 fp32, 0.993 bf16 (both h0)."""
    N, S = 33, 32
    M = N * S
    rays, zs, rd, zd, dn_dev, dn = _inputs(N, S)
    net = TL._net(A, "mip", "he")
    worst, layers, detail, padding = {}, {}, {}, []
    for fam in G.FAMILIES:
        out, dump = _train_forward(A, net, prec, rd, S, zd[fam], dn_dev, A.ops.CONTRACT_GAUSSIAN)
        out1, dump1 = _train_forward(A, net, prec, rd, S, zd[fam], dn_dev, True)
        mu, feat = _encoding_slot(A, net, prec, M, dump)
        mu1, feat1 = _encoding_slot(A, net, prec, M, dump1)
        b = G.kernel_bounds(zs[fam], rays, 10, R2, dn, path="doubling" if prec == "bf16" else "direct", stored_bf16=prec == "bf16")
        rep = G.compare(b, feat.reshape(N, S, 60), mu.reshape(N, S, 3), twin=(feat1.reshape(N, S, 60), mu1.reshape(N, S, 3)))
        print("training forward %s %s: %s" % (prec, fam, rep))
        _merge(worst, rep)
        TL._check_run(A, net, prec, M, out.reshape(M, 4), dump, layers, detail, "ipe-gaussian %s M=%d" % (fam, M), padding)
        del dump, dump1
    _emit("ipe-gaussian fwd mip %s he encoding" % prec, worst)
    TL._emit("fwd-layers mip %s he ipe-gaussian" % prec, layers, detail)
    assert not padding, "\n".join(padding)


# ------------------------------------------------------------------------------------------------ 3: render == training forward
def _mixed(zs):
    """ray i takes its depths from family i % 3"""
    z = zs["inside"].clone()
    for k, fam in enumerate(G.FAMILIES):
        z[k::3] = zs[fam][k::3]
    return z.cuda().contiguous()


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_render_kernel_equals_the_training_forward_bit_for_bit(A, prec):
    net = TL._net(A, "mip", "he")
    P = TL._code(A, prec)
    for M in (1, 63, 64, 65, 1056, 3 * A.n_cu * F.TILE[prec] + 77):
        N, S = TL._ray_split(M)
        rays, zs, rd, _, dn_dev, dn = _inputs(N, S, need_gap=False)
        z = _mixed(zs)
        what = "%s M=%d (%d x %d)" % (prec, M, N, S)
        out, dump = _train_forward(A, net, prec, rd, S, z, dn_dev, A.ops.CONTRACT_GAUSSIAN)
        del dump
        got = A.ops.mip_forward_samples(net.packed(A, prec), P, _descriptor(A, rd, S, z, dn_dev, A.ops.CONTRACT_GAUSSIAN), (N, S), "cuda")
        _same_bits(got, out, what + ": render kernel against the training forward")
        assert bool(torch.isfinite(out).all()), what
        if prec == "bf16":
            out8, dump8 = _train_forward(A, net, prec, rd, S, z, dn_dev, A.ops.CONTRACT_GAUSSIAN, fmt="fp8")
            del dump8
            _same_bits(out8, out, what + ": fp8-dump training forward")
        if M >= 63:
            one = A.ops.mip_forward_samples(net.packed(A, prec), P, _descriptor(A, rd, S, z, dn_dev, True), (N, S), "cuda")
            assert not torch.equal(one, got), what + ": the Gaussian mode is not on"


# ------------------------------------------------------------------------------------------------ 4: inside the ball
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inside_the_ball_the_mode_is_contract_1_bit_for_bit(A, prec):
    N, S = 33, 32
    M = N * S
    rays, zs, rd, zd, dn_dev, dn = _inputs(N, S)
    assert bool(G.kernel_bounds(zs["inside"], rays, 10, R2, dn)["inside"].all())
    assert float((rays[:, None, :3].double() + zs["inside"][..., None].double() * rays[:, None, 3:].double()).norm(dim=-1).max()) < 1.0
    net = TL._net(A, "mip", "he")
    P = TL._code(A, prec)
    res = {}
    for c in (True, A.ops.CONTRACT_GAUSSIAN):
        out, dump = _train_forward(A, net, prec, rd, S, zd["inside"], dn_dev, c)
        _, enc, _ = TL._read(A, net, prec, M, dump)
        res[c] = (out, enc, A.ops.mip_forward_samples(net.packed(A, prec), P, _descriptor(A, rd, S, zd["inside"], dn_dev, c), (N, S), "cuda"))
        del dump
    for a, b, what in zip(res[True], res[A.ops.CONTRACT_GAUSSIAN], ("training rgbo", "encoding slot", "render rgbo")):
        _same_bits(a, b, "%s inside the ball: %s" % (prec, what))
    if prec == "fp32":
        for L in (10, 4):
            one = A.ops.ipe_feature(zd["inside"], rd, L, RADIUS, dn_dev, contract=True)
            two = A.ops.ipe_feature(zd["inside"], rd, L, RADIUS, dn_dev, contract=A.ops.CONTRACT_GAUSSIAN)
            for a, b, what in zip(one, two, ("feat", "mu", "mu_t")):
                _same_bits(a, b, "encoder L=%d inside the ball: %s" % (L, what))


# ------------------------------------------------------------------------------------------------ 5: far rays
def _att2_with_slack(feat, b, L):
    """sin^2 + cos^2 per (level, coordinate) from what the kernel wrote, and the derived bound on its distance from the exact
    att^2: every feature is within e of its exact value v, so |got^2 - v^2| <= 2 |v| e + e^2"""
    N, S = feat.shape[:2]
    e = (2 * b.v.abs() * b.e + b.e * b.e).reshape(N, S, L, 2, 3).sum(3)
    return G.att2(feat, L), e


def test_far_rays_keep_the_mean_and_gain_attenuation(A):
    N, S, L = 33, 32, 10
    rays, zs, rd, zd, dn_dev, dn = _inputs(N, S)
    for fam in ("straddle", "far"):
        z, zc = zs[fam], zd[fam]
        g = [t.cpu() for t in A.ops.ipe_feature(zc, rd, L, RADIUS, dn_dev, contract=A.ops.CONTRACT_GAUSSIAN)]
        m = [t.cpu() for t in A.ops.ipe_feature(zc, rd, L, RADIUS, dn_dev, contract=True)]
        assert not torch.equal(g[0], m[0]), fam
        _same_bits(g[1], m[1], fam + ": mu")
        bg, bm = G.kernel_bounds(z, rays, L, R2, dn)["feat"], G.kernel_bounds(z, rays, L, R2, dn, mode="metric")["feat"]
        ag, eg = _att2_with_slack(g[0], bg, L)
        am, em = _att2_with_slack(m[0], bm, L)
        short = ((am - em).clamp_min(0).prod(-1) - (ag + eg).prod(-1)).max()
        print("%s: prod_c att^2 (metric, lower) - prod_c att^2 (gaussian, upper), max %.3e" % (fam, float(short)))
        assert float(short) <= 0.0, fam
        assert float((ag.prod(-1) - am.prod(-1)).max()) > 0.1, fam                 # the gain is not a rounding effect
        # rays through the origin: element by element
        r0 = G.radial(rays)
        assert G.sphere_gap(z, r0) >= G.SPHERE_GAP
        r0d = r0.cuda()
        g0 = A.ops.ipe_feature(zc, r0d, L, RADIUS, dn_dev, contract=A.ops.CONTRACT_GAUSSIAN)[0].cpu().double()
        m0 = A.ops.ipe_feature(zc, r0d, L, RADIUS, dn_dev, contract=True)[0].cpu().double()
        slack = G.kernel_bounds(z, r0, L, R2, dn)["feat"].e + G.kernel_bounds(z, r0, L, R2, dn, mode="metric")["feat"].e
        short = (m0.abs() - g0.abs() - slack).max()
        print("%s, rays through the origin: |feat_metric| - |feat_gaussian| - rounding, max %.3e" % (fam, float(short)))
        assert float(short) <= 0.0, fam
        assert float((g0.abs() - m0.abs()).max()) > 0.1, fam


# ------------------------------------------------------------------------------------------------ 6: routes
SIDE, NF = 30, 32                                        # 30: the smallest width procedures.get_patch_size tiles (one 30 x 30 tile)


def _render_nets(hidden=256):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, hidden)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small", hidden=hidden) if hidden != 256 else W.mip_state("small"))
    return prop.cuda().eval(), mip.cuda().eval()


def _camera():
    return O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda(), O.fov2focal(0.6911112070083618, (SIDE, SIDE))


ROUTES = {"plain": dict(near=0.5, far=8.0), "warped": dict(near=0.2, far=1e6, spacing="disparity"),
          "rounds": dict(near=0.2, far=1e6, spacing="disparity", prop_rounds=2, prop_pnum=48)}


@pytest.mark.parametrize("route", list(ROUTES))
def test_render_image_routes_equal_the_call_by_call_route(A, route):
    """the tolerance of the existing fused-against-by-calls integrated-PE comparisons (test_gpu_two_round_render: IPE_ROUTE_FIGURE =
    0.0): the two routes run the same kernels on the same Philox streams, bit for bit"""
    from nerf_amd import procedures, utils
    from nerf_amd.procedures import render_image
    assert procedures.get_patch_size((SIDE, SIDE)) == (SIDE, (1, 1)) and all(procedures.get_patch_size((w, w))[0] is None for w in range(1, SIDE))
    kw = dict(ROUTES[route])
    near, far = kw.pop("near"), kw.pop("far")
    prop, mip = _render_nets()
    pose, focal = _camera()
    assert procedures._render_route(False, False, kw.get("spacing") == "disparity", kw.get("prop_rounds", 1), kw.get("prop_pnum", 64)) == route
    fx, fy = utils._focal_xy(focal)
    rays = A.ops.generate_rays(pose, SIDE, SIDE, fx, fy, pose.device)                # one tile: tile order is raster order
    with torch.no_grad():
        img = render_image(mip, prop, pose, SIDE, focal, near, far, NF, white_bkg=True, render_depth=True, ipe=True, contract=True, seed=SEED,
                           ipe_cov="contracted", **kw)
        metric = render_image(mip, prop, pose, SIDE, focal, near, far, NF, white_bkg=True, render_depth=True, ipe=True, contract=True, seed=SEED, **kw)
        z_base = torch.linspace(near, far, 64, device="cpu").cuda()
        rgb, depth, _ = procedures._render_rays_by_calls(mip, prop, rays, z_base, None, None, NF, near, far, True, True, seed=SEED, contract=True,
                                                         ipe_radius=2.0 / 12.0 ** 0.5 / fx, ipe_dir_norm=A.ops.dirs_norm(rays), ipe_cov="contracted", **kw)
    got_rgb, got_depth = img["rgb"].permute(1, 2, 0).reshape(-1, 3), img["depth_img"][0].reshape(-1)
    print("%s: fused vs by-calls rgb %.3e depth %.3e; contracted vs metric covariance rgb %.3e" % (
        route, max_abs(got_rgb, rgb), max_abs(got_depth, depth), max_abs(img["rgb"], metric["rgb"])))
    assert bool(torch.isfinite(img["rgb"]).all()) and bool(torch.isfinite(img["depth_img"]).all())
    assert torch.equal(got_rgb, rgb) and torch.equal(got_depth, depth), route
    assert not torch.equal(img["rgb"], metric["rgb"]), route                        # the covariance really is contracted


def test_layer_by_layer_route_and_shards(A):
    """hidden width 320 (the generic shape the suite's weights exist for): the stand-alone encoder feeds the layers.  On five rays the
    network's output equals the oracle's network on the SPECIFICATION's [mu' | feat] within the 1e-4 of the existing generic-route
    integrated-PE comparisons (test_gpu_parity); then three shards of each route's image, stitched, are the image bit for bit."""
    from nerf_amd import parallel
    from nerf_amd.procedures import render_image
    prop, wide = _render_nets(hidden=320)
    assert wide._generic()
    rays, zs, rd, zd, dn_dev, dn = _inputs(5, 3)
    sd = {k: v.detach().cpu().double() for k, v in wide.state_dict().items()}
    with torch.no_grad():
        for fam in G.FAMILIES:
            got = wide.forward_rays(rd, zd[fam], 3, ipe_radius=RADIUS, ipe_dir_norm=dn_dev, contract=True, ipe_cov="contracted").cpu().double()
            feat, mu, _ = G.spec(zs[fam], rays, 10, R2, dn)
            pts = torch.cat((mu, rays[:, None, 3:].double().expand(-1, 3, -1)), -1)
            want = O.mip_forward(sd, pts, encoded_x=feat)
            gate("layer-by-layer ipe_cov='contracted' %s: rgbo vs oracle network on the fp64 specification" % fam,
                 max_abs(got, want) / max(1.0, float(want.abs().max())), 1e-4)
            if fam != "inside":
                one = wide.forward_rays(rd, zd[fam], 3, ipe_radius=RADIUS, ipe_dir_norm=dn_dev, contract=True).cpu().double()
                assert not torch.equal(one, got), fam
    pose, focal = _camera()
    _, mip = _render_nets()
    with torch.no_grad():
        for net, kw in ((wide, dict(ROUTES["warped"])), (mip, dict(ROUTES["rounds"])), (mip, dict(ROUTES["plain"]))):
            kw.update(white_bkg=True, render_depth=True, ipe=True, contract=True, seed=SEED, ipe_cov="contracted")
            near, far = kw.pop("near"), kw.pop("far")
            one = render_image(net, prop, pose, SIDE, focal, near, far, NF, **kw)
            assert bool(torch.isfinite(one["rgb"]).all())
            parts = [render_image(net, prop, pose, SIDE, focal, near, far, NF, _shard=parallel.shard_range(SIDE * SIDE, r, 3, align=256), **kw)
                     for r in range(3)]
            ranges = [q["range"] for q in parts]
            assert ranges[0][0] == 0 and ranges[2][1] == SIDE * SIDE and all(a[1] == b[0] and a[0] < a[1] for a, b in zip(ranges, ranges[1:]))
            rgb3 = parts[0]["to_image"](torch.cat([q["rgb_rays"] for q in parts]), 3)
            dep3 = parts[0]["to_image"](torch.cat([q["depth_rays"] for q in parts]).unsqueeze(-1), 1)
            assert torch.equal(rgb3, one["rgb"]) and torch.equal(dep3.expand(3, -1, -1), one["depth_img"])


# ------------------------------------------------------------------------------------------------ 7: the training step
def _train_step(near, far, radius_pose, **kw):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small"))
    prop, mip = prop.cuda().train(), mip.cuda().train()
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=1e-5, lr_on_device=True)
    st = TrainStep(prop, mip, opt, (24, 32), (30.0, 28.0), near, far, ray_num=64, coarse_pnum=16, fine_pnum=32, seed=1234, ipe_radius=2.0 / 12.0 ** 0.5 / 30.0,
                   contract=True, **kw)
    gen = torch.Generator().manual_seed(4)
    st.set_image(torch.rand(3, 24, 32, generator=gen).cuda(), O.pose_spherical(30.0, -30.0, radius_pose)[:3].contiguous().cuda())
    return st, prop, mip


def _params(prop, mip):
    return [p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())]


def test_train_step_replayed_equals_eager(A):
    res = []
    for graphed in (False, True):
        st, prop, mip = _train_step(0.2, 1e6, 4.0, spacing="disparity", ipe_cov="contracted")
        if graphed:
            st.capture(warmup=2)
            for _ in range(2):
                st()
        else:
            for _ in range(4):
                st()
        torch.cuda.synchronize()
        assert torch.isfinite(st.loss).item()
        res.append(_params(prop, mip))
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_train_step_inside_the_ball_and_far(A):
    """inside: the camera 0.3 from the origin, depths 0.05 .. 0.4, |d| <= 1.21: every frustum within 0.3 + 0.4 x 1.21 < 1 of the origin, so
    the flat gradient buffer after one iteration is the metric mode's bit for bit.  far: 0.2 .. 1e6 in disparity, the loss is finite
    and another number."""
    out = {}
    for name, (near, far, rp, kw) in {"inside": (0.05, 0.4, 0.3, {}), "far": (0.2, 1e6, 4.0, dict(spacing="disparity"))}.items():
        for cov in ("metric", "contracted"):
            st, prop, mip = _train_step(near, far, rp, ipe_cov=cov, **kw)
            loss, img_loss = st()
            torch.cuda.synchronize()
            assert math.isfinite(float(loss)) and math.isfinite(float(img_loss)), (name, cov)
            assert st.flat_grads is not None and float(st.flat_grads.flat.abs().max()) > 0.0
            out[(name, cov)] = (st.flat_grads.flat.detach().clone(), float(loss), _params(prop, mip))
    a, b = out[("inside", "metric")], out[("inside", "contracted")]
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and a[1] == b[1] and all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    a, b = out[("far", "metric")], out[("far", "contracted")]
    print("far: loss %.9g (metric covariance) %.9g (contracted covariance)" % (a[1], b[1]))
    assert a[1] != b[1] and not torch.equal(a[0], b[0])
