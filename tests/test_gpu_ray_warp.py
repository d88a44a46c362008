"""Disparity ray spacing (Mip-NeRF 360's normalised distance s) on the device: every new kernel stage by stage against the specification
in tests/ray_warp_ref.py, the fused render entry point end to end, the call-by-call route, `spacing="linear"` leaving every existing
result bit for bit, and the training step.  The reference has no such code: the definition is the build's own (include/nerf_amd.h)."""
import math

import pytest
import torch
import torch.nn.functional as F

import ray_warp_ref as R
import weights as W
from conftest import gate, max_abs
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
PAIRS = ((2.0, 6.0), (0.2, 1000.0))
N_RAYS = 7                                                   # not a multiple of the 4 rays / waves of a workgroup


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def _rays(n, seed, spread=0.25, origin=(0.0, 0.0, 1.5)):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor(origin).expand(n, 3)
    d = torch.randn(n, 3, generator=g) * spread + torch.tensor([0.0, 0.0, -1.0])
    d = d * (0.7 + 0.6 * torch.rand(n, 1, generator=g))      # un-normalised directions, like the reference's rays
    return torch.cat((o, d), -1).contiguous(), g


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nets(train=False, hidden=256):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, hidden)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small", hidden=hidden) if hidden != 256 else W.mip_state("small"))
    prop, mip = prop.cuda(), mip.cuda()
    return (prop.train(), mip.train()) if train else (prop.eval(), mip.eval())


def _ref_net(train=False):
    from nerf_amd.ref_model import RefNeRF
    net = RefNeRF(10, 4)
    net.load_state_dict(W.ref_state("small"))
    net = net.cuda()
    return net.train() if train else net.eval()


# ------------------------------------------------------------------------------------------------ 3. warp_depths
@pytest.mark.parametrize("near,far", PAIRS)
def test_warp_depths_against_the_fp64_spec(near, far):
    """Forward |z - z64| <= 8 2^-24 z64 (five roundings of positive terms, room for a division that is not correctly rounded); inverse
    8 2^-24 / (1 - near/far) absolute (the cancellation in 1/z - gn over gf - gn); pts within 2 2^-24 (|o| + |z d|) per component of the
    fp64 value formed from the kernel's own z (one product, one sum)."""
    from nerf_amd import ops, utils
    rays, g = _rays(N_RAYS, 11)
    for S in (1, 65):
        s = torch.rand(N_RAYS, S, generator=g) * 1.5 - 0.25                          # a quarter of them outside [0, 1]: clamped
        s[0, 0], s[-1, -1] = 0.0, 1.0
        z, pts = ops.warp_depths(s.cuda(), near, far, rays.cuda())
        z64 = R.warp(s.double(), near, far)
        gate("warp_depths forward (%g, %g) S=%d: relative to fp64, in 2^-24" % (near, far, S), float(((z.cpu().double() - z64).abs() / z64).max()) / EPS, 8.0)
        assert _same_bits(z, R.warp(s, near, far))                                   # ... and the fp32 spec bit for bit
        assert float(z.min()) >= near * (1 - 4 * EPS) and float(z.max()) <= far * (1 + 4 * EPS)
        zz = z.cpu().double()
        want = rays[:, None, :3].double() + rays[:, None, 3:].double() * zz[:, :, None]
        room = rays[:, None, :3].double().abs() + (rays[:, None, 3:].double() * zz[:, :, None]).abs()
        gate("warp_depths pts (%g, %g) S=%d: of 2^-24 (|o| + |z d|)" % (near, far, S), float(((pts.cpu().double() - want).abs() / room).max()) / EPS, 2.0)
        zin = torch.cat((z.cpu(), torch.tensor([[near * 0.5, far * 2.0]]).expand(N_RAYS, 2)), -1).contiguous()      # + two outside [near, far]
        back, none = ops.warp_depths(zin.cuda(), near, far, inverse=True)
        assert none is None
        s64 = R.unwarp(zin.double(), near, far)
        gate("warp_depths inverse (%g, %g) S=%d: absolute, in 2^-24 / (1 - near/far)" % (near, far, S),
             float((back.cpu().double() - s64).abs().max()) / EPS * (1.0 - near / far), 8.0)
        assert _same_bits(back, R.unwarp(zin, near, far))
        assert _same_bits(utils.warp_depths(s.cuda(), near, far, "disparity"), z) and _same_bits(utils.unwarp_depths(zin.cuda(), near, far, "disparity"), back)
    z0, p0 = ops.warp_depths(torch.empty(0, 5, device="cuda"), near, far, torch.empty(0, 6, device="cuda"))
    assert tuple(z0.shape) == (0, 5) and tuple(p0.shape) == (0, 5, 3)
    with pytest.raises(Exception):
        ops.warp_depths(torch.rand(2, 3).cuda(), near, far, spacing="linear")        # the kernel entry points take the disparity kind only


# ------------------------------------------------------------------------------------------------ 4. warped_stratified
@pytest.mark.parametrize("near,far", PAIRS)
def test_warped_stratified_draw(near, far):
    from nerf_amd import ops
    rays, g = _rays(N_RAYS, 12)
    Rc = rays.cuda()
    for C in (32, 64, 130):
        u = torch.rand(N_RAYS, C, generator=g)
        u[0, -1] = 1.0 - EPS                                                          # the largest draw: s = 1.0 at C = 64
        s_c, z_c, pts = ops.warped_stratified(Rc, u.cuda(), near, far)
        assert _same_bits(s_c, R.coarse_s(u)), C
        z_w, p_w = ops.warp_depths(s_c, near, far, Rc)
        assert _same_bits(z_c, z_w) and _same_bits(pts, p_w), C
        assert float(s_c.max()) <= 1.0
    for C in (32, 64):                                                                # in-kernel Philox: word 0 of the 'RS' blocks, 64 slots per ray
        for off in (0, 2 ** 33 + 5):
            u = ops.philox_stream((N_RAYS, C), 987654321, off, strat=True, device="cuda")
            a = ops.warped_stratified(Rc, None, near, far, n_points=C, seed=987654321, ray_offset=off)
            b = ops.warped_stratified(Rc, u, near, far)
            assert all(_same_bits(x, y) for x, y in zip(a, b)), (C, off)
            assert _same_bits(u.cpu(), O.philox_uniforms(987654321, N_RAYS, off, C, 1)[0])
    with pytest.raises(Exception):
        ops.warped_stratified(Rc, None, near, far, n_points=130, seed=1)


# ------------------------------------------------------------------------------------------------ 5. warped_resample
def _resample_inputs(C, K, seed):
    rays, g = _rays(N_RAYS, seed)
    u_c = torch.rand(N_RAYS, C, generator=g)
    s_c = R.coarse_s(u_c)
    s_c[2, [3, 5]] = s_c[2, [5, 3]]                                                   # ray 2: explicit s_c that is not ascending (nor are its bins)
    density = torch.randn(N_RAYS, C, generator=g) * 2.0
    density[1] = -5.0
    density[1, C // 3] = 400.0                                                        # ray 1: one very dense sample takes all the mass
    u = torch.rand(N_RAYS, K, generator=g)
    u[3] = 0.5 + torch.rand(K, generator=g) / 300.0                                   # ray 3: every draw in one or two of the sort's 256 buckets -> rank-sort fallback
    return rays, s_c.contiguous(), density, u


@pytest.mark.parametrize("softplus", [False, True])
@pytest.mark.parametrize("C,K", [(32, 65), (64, 129), (130, 200)])
@pytest.mark.parametrize("near,far", PAIRS)
def test_warped_resample_equals_the_chain_of_ops_and_the_spec(near, far, C, K, softplus):
    from nerf_amd import ops
    rays, s_c, density, u = _resample_inputs(C, K, 100 + C)
    Rc, Sc, Dc, Uc = rays.cuda(), s_c.cuda(), density.cuda(), u.cuda()
    z_f, s_f, below, w_prop = ops.warped_resample(Dc, Sc, Rc, Uc, near, far, softplus=softplus)
    # the chain of existing ops on the same inputs: the fused kernel shares their device functions
    z_c = ops.warp_depths(Sc, near, far)[0]
    w = ops.max_blur(ops.sigma_to_weights(Dc, z_c, Rc[:, 3:].contiguous(), ops.ACT_SOFTPLUS if softplus else ops.ACT_RELU), 0.01)
    s_chain, below_chain = ops.inverse_sample(w, Sc, Uc, sort=True)
    z_chain = ops.warp_depths(s_chain, near, far)[0]
    assert _same_bits(w_prop, w) and _same_bits(s_f, s_chain) and torch.equal(below, below_chain) and _same_bits(z_f, z_chain)
    assert bool((s_f[:, 1:] >= s_f[:, :-1]).all())
    # in-kernel inverse-CDF uniforms == the explicit Philox tensor
    for off in (0, 2 ** 33 + 5):
        up = ops.philox_stream((N_RAYS, K), 4242, off, device="cuda")
        a = ops.warped_resample(Dc, Sc, Rc, None, near, far, K=K, softplus=softplus, seed=4242, ray_offset=off)
        b = ops.warped_resample(Dc, Sc, Rc, up, near, far, softplus=softplus)
        assert all(_same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b)), off
    # optional outputs may be skipped
    only = ops.warped_resample(Dc, Sc, Rc, Uc, near, far, softplus=softplus, want_s=False, want_below=False, want_w=False)
    assert _same_bits(only[0], z_f) and only[1] is None and only[2] is None and only[3] is None
    # against the CPU specification fed the HIP density
    w_spec = R.proposal_weights(density, s_c, rays[:, 3:], near, far, softplus=softplus)
    s_spec, below_spec, _ = R.resample(w_spec, s_c, u, near, far)
    gate("warped_resample s_fine vs CPU spec (%g, %g) C=%d K=%d softplus=%d" % (near, far, C, K, softplus), max_abs(s_f.cpu(), s_spec), 5e-6)
    gate("warped_resample share of differing below (%g, %g) C=%d K=%d softplus=%d" % (near, far, C, K, softplus),
         float((below.cpu() != below_spec).float().mean()), 0.01)


# ------------------------------------------------------------------------------------------------ 6. the fused entry point
def _camera_rays(H, Wd, n):
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3]
    focal = O.fov2focal(0.6911112070083618, (H, Wd))
    dirs = O.ray_dirs_image(pose, H, Wd, focal).reshape(-1, 3)
    rays = torch.cat((pose[:, -1].expand(H * Wd, -1), dirs), -1).contiguous()
    pick = torch.randperm(H * Wd, generator=torch.Generator().manual_seed(8))[:n]
    return rays[pick].contiguous()


def test_render_rays_warped_against_the_spec():
    """200 rays of a 40 x 40 camera, 64 + 128 samples, (near, far) = (0.2, 1000), 'small' weights, fp32, contracted: rgb, weights and the
    s-depth within the project's end-to-end fp32 gate 1e-4 of the specification; a slice rendered with rng_ray_offset equals the rows of the
    whole; the white-background identity."""
    from nerf_amd import ops
    near, far, n, nf = 0.2, 1000.0, 200, 128
    prop, mip = _nets()
    rays = _camera_rays(40, 40, n)
    g = torch.Generator().manual_seed(21)
    u1, u2 = torch.rand(n, 64, generator=g), torch.rand(n, nf + 1, generator=g)
    P = ops.F32
    pk_p, pk_m = prop.packed(P), mip.packed(P)
    rgb, depth, w, ws = ops.render_rays_warped(pk_p, pk_m, P, rays.cuda(), u1.cuda(), u2.cuda(), nf, near, far, True, want_depth=True, want_weights=True,
                                               contract=True)
    with torch.no_grad():
        want_rgb, want_w, want_d = R.render_rays(W.proposal_state("small"), W.mip_state("small"), rays, u1, u2, near, far, nf, white_bkg=True, contracted=True)
    gate("render_rays_warped rgb vs spec", max_abs(rgb.cpu(), want_rgb), 1e-4)
    gate("render_rays_warped weights vs spec", max_abs(w.cpu(), want_w), 1e-4)
    gate("render_rays_warped s-depth vs spec", max_abs(depth.cpu(), want_d), 1e-4)
    assert float(depth.min()) >= 0.0 and float(depth.max()) <= 1.0
    # in-kernel Philox: the same as the explicit streams, and a shard reproduces the rows of the whole
    Rc = rays.cuda()
    rgb_w, depth_w, w_w, ws = ops.render_rays_warped(pk_p, pk_m, P, Rc, None, None, nf, near, far, True, want_weights=True, contract=True, seed=77, workspace=ws)
    p1, p2 = ops.philox_stream((n, 64), 77, 0, strat=True, device="cuda"), ops.philox_stream((n, nf + 1), 77, 0, device="cuda")
    rgb_e, depth_e, _, _ = ops.render_rays_warped(pk_p, pk_m, P, Rc, p1, p2, nf, near, far, True, contract=True)
    assert torch.equal(rgb_e, rgb_w) and torch.equal(depth_e, depth_w)
    lo, hi = 61, 150
    rgb_s, depth_s, _, _ = ops.render_rays_warped(pk_p, pk_m, P, Rc[lo:hi].contiguous(), None, None, nf, near, far, True, contract=True, seed=77, rng_ray_offset=lo)
    assert torch.equal(rgb_s, rgb_w[lo:hi]) and torch.equal(depth_s, depth_w[lo:hi])
    rgb_b, _, _, _ = ops.render_rays_warped(pk_p, pk_m, P, Rc, None, None, nf, near, far, False, contract=True, seed=77)
    acc = w_w.sum(-1)
    assert float(acc.max()) <= 1.0 + 1e-4 and float(w_w.min()) >= 0.0
    assert max_abs(rgb_w - rgb_b, (1.0 - acc)[:, None].expand(-1, 3)) <= 2e-6
    rgb_plain, _, _, _ = ops.render_rays_warped(pk_p, pk_m, P, Rc, None, None, nf, near, far, True, seed=77)
    assert float((rgb_plain - rgb_w).abs().max()) > 1e-5                              # the contraction is really on (fp32 noise between equal computations: ~1e-7)


def test_render_rays_warped_with_integrated_pe_against_the_spec():
    """The same rays with the integrated PE in the fine pass (frusta between the 129 consecutive METRIC fine depths, contracted means),
    against ray_warp_ref.render_rays(ipe_radius=...): the end-to-end fp32 gate 1e-4 (the fp32 spec is 1.4e-7 / 1.1e-6 / 1.1e-7 from
    its own fp64 evaluation on 64 of these rays).  200 rays take the direction norm through the scratch partials, 5 rays through the
    one-block kernel (both leave it in the workspace tail); a shard handed the whole list's norm reproduces the rows of the whole; and
    the training step takes ipe_radius under disparity spacing."""
    from nerf_amd import ops
    near, far, nf = 0.2, 1000.0, 128
    radius = 2.0 / math.sqrt(12.0) / 55.0
    prop, mip = _nets()
    P = ops.F32
    pk_p, pk_m = prop.packed(P), mip.packed(P, wide=True)
    rays = _camera_rays(40, 40, 200)
    g = torch.Generator().manual_seed(22)
    u1, u2 = torch.rand(200, 64, generator=g), torch.rand(200, nf + 1, generator=g)
    for n in (200, 5):
        r, a, b = rays[:n].contiguous(), u1[:n].contiguous(), u2[:n].contiguous()
        rgb, depth, w, _ = ops.render_rays_warped(pk_p, pk_m, P, r.cuda(), a.cuda(), b.cuda(), nf, near, far, True, want_depth=True, want_weights=True,
                                                  contract=True, ipe_radius=radius)
        with torch.no_grad():
            want_rgb, want_w, want_d = R.render_rays(W.proposal_state("small"), W.mip_state("small"), r, a, b, near, far, nf, white_bkg=True, contracted=True,
                                                     ipe_radius=radius)
        gate("render_rays_warped + IPE, %d rays: rgb vs spec" % n, max_abs(rgb.cpu(), want_rgb), 1e-4)
        gate("render_rays_warped + IPE, %d rays: weights vs spec" % n, max_abs(w.cpu(), want_w), 1e-4)
        gate("render_rays_warped + IPE, %d rays: s-depth vs spec" % n, max_abs(depth.cpu(), want_d), 1e-4)
        if n == 200:
            whole = rgb
            plain, _, _, _ = ops.render_rays_warped(pk_p, pk_m, P, r.cuda(), a.cuda(), b.cuda(), nf, near, far, True, contract=True)
            assert float((plain - rgb).abs().max()) > 1e-6                            # the integrated PE is really on
    Rc = rays.cuda()
    part, _, _, _ = ops.render_rays_warped(pk_p, pk_m, P, Rc[40:90].contiguous(), u1[40:90].cuda(), u2[40:90].cuda(), nf, near, far, True, contract=True,
                                           ipe_radius=radius, ipe_dir_norm=ops.dirs_norm(Rc))
    assert torch.equal(part, whole[40:90])
    prop_t, mip_t = _nets(train=True)
    st = _step9(prop_t, mip_t, ray_num=96, coarse_pnum=32, fine_pnum=64, ipe_radius=radius, distortion=0.01, lr=1e-5)
    loss, img_loss = st()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and math.isfinite(float(img_loss)) and float(st.dist_loss) > 0.0
    assert all(bool(torch.isfinite(p).all()) for p in list(mip_t.parameters()) + list(prop_t.parameters()))


# ------------------------------------------------------------------------------------------------ 7. fused route against the call-by-call route
def _routes(spacing, near, far, seed=2024, H=50, Wd=50, nf=128):
    """(render_image's rgb, depth as ray lists) and the same from _render_rays_by_calls on the explicit Philox tensors"""
    from nerf_amd import ops, procedures, utils
    prop, mip = _nets()
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (H, Wd))
    with torch.no_grad():
        img = procedures.render_image(mip, prop, pose, (H, Wd), focal, near, far, nf, white_bkg=True, render_depth=True, contract=True, seed=seed, spacing=spacing)
        fx, fy = utils._focal_xy(focal)
        rays = ops.generate_rays(pose, H, Wd, fx, fy, pose.device)                          # one 50 x 50 tile: tile order is raster order
        n = H * Wd
        u1, u2 = ops.philox_stream((n, 64), seed, 0, strat=True, device="cuda"), ops.philox_stream((n, nf + 1), seed, 0, device="cuda")
        z_base = torch.linspace(near, far, 64).cuda()
        rgb, depth, _ = procedures._render_rays_by_calls(mip, prop, rays, z_base, u1, u2, nf, near, far, True, True, contract=True, spacing=spacing)
    return img["rgb"].permute(1, 2, 0).reshape(-1, 3), img["depth_img"][0].reshape(-1), rgb, depth


# The same comparison under spacing="linear" -- code this change does not touch, so the figure is the parent commit's -- measured on an
# MI355X: rgb 0.0, depth 0.0 (the two routes agree bit for bit: the MLP kernels are fed identical positions).  Hence bit equality here.
LINEAR_ROUTE_FIGURE = (0.0, 0.0)


def test_fused_route_against_the_call_by_call_route():
    """render_image(spacing="disparity") on a 50 x 50 image against _render_rays_by_calls(spacing="disparity") on the explicit Philox
    tensors.  Yardstick: the same comparison under spacing="linear" (code this change does not touch; re-measured in the same run).
    Measured: linear rgb 0.0 / depth 0.0, so the two routes must agree bit for bit under disparity spacing too (measured: they do)."""
    fr, fd, cr, cd = _routes("linear", 2.0, 6.0)
    lin_rgb, lin_d = max_abs(fr, cr), max_abs(fd, cd)
    print("fused vs by-calls, linear (2, 6): rgb %.3e depth %.3e" % (lin_rgb, lin_d))
    fr, fd, cr, cd = _routes("disparity", 0.2, 1000.0)
    dis_rgb, dis_d = max_abs(fr, cr), max_abs(fd, cd)
    print("fused vs by-calls, disparity (0.2, 1000): rgb %.3e depth %.3e" % (dis_rgb, dis_d))
    assert bool(torch.isfinite(fr).all()) and bool(torch.isfinite(fd).all())
    assert LINEAR_ROUTE_FIGURE is not None
    if LINEAR_ROUTE_FIGURE == (0.0, 0.0):
        assert lin_rgb == 0.0 and lin_d == 0.0
        assert torch.equal(fr, cr) and torch.equal(fd, cd)
    else:
        gate("fused vs by-calls under disparity spacing: rgb", dis_rgb, 2.0 * LINEAR_ROUTE_FIGURE[0])
        gate("fused vs by-calls under disparity spacing: depth", dis_d, 2.0 * LINEAR_ROUTE_FIGURE[1])


def test_generic_width_and_refnerf_render_under_disparity_spacing():
    from nerf_amd import procedures
    near, far = 0.2, 1000.0
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (50, 50))
    prop, mip320 = _nets(hidden=320)
    assert mip320._generic()
    outs = []
    with torch.no_grad():
        for _ in range(2):
            torch.manual_seed(5)
            outs.append(procedures.render_image(mip320, prop, pose, 50, focal, near, far, 64, white_bkg=True, render_depth=True, contract=True, spacing="disparity"))
    assert torch.equal(outs[0]["rgb"], outs[1]["rgb"]) and torch.equal(outs[0]["depth_img"], outs[1]["depth_img"])
    assert bool(torch.isfinite(outs[0]["rgb"]).all()) and float(outs[0]["depth_img"].min()) >= 0.0 and float(outs[0]["depth_img"].max()) <= 1.0
    ref = _ref_net()
    with torch.no_grad():
        a = procedures.render_image(ref, prop, pose, 50, focal, near, far, 64, white_bkg=True, render_depth=True, render_normal=True, seed=9, spacing="disparity")
        b = procedures.render_image(ref, prop, pose, 50, focal, near, far, 64, white_bkg=False, seed=9, spacing="disparity")
    assert all(bool(torch.isfinite(a[k]).all()) for k in ("rgb", "depth_img", "normal_img"))
    acc = 1.0 - (a["rgb"] - b["rgb"])                                                 # white background adds 1 - sum w to every channel
    assert float(acc.max()) <= 1.0 + 1e-4 and float(acc.min()) >= -1e-4
    assert float(a["depth_img"].min()) >= 0.0 and float(a["depth_img"].max()) <= 1.0


# ------------------------------------------------------------------------------------------------ 8. nothing existing moves
def _scene_stack(V=4, H=24, Wd=32, seed=4, lo=0.0, hi=1.0):
    gen = torch.Generator().manual_seed(seed)
    blocks = lo + (hi - lo) * torch.rand(V, 3, 4, 1, 4, 1, generator=gen)                                                           # colour blocks
    blocks = blocks.expand(V, 3, 4, H // 4, 4, Wd // 4).reshape(V, 3, H, Wd).contiguous()
    poses = torch.stack([O.pose_spherical(20.0 + 40.0 * v, -25.0, 1.5)[:3] for v in range(V)]).contiguous()
    return blocks.cuda(), poses.cuda()


def _train_step(prop, net, near, far, lr=5e-4, scene=None, **kw):
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    opt = Adam(list(net.parameters()) + list(prop.parameters()), lr=lr, lr_on_device=True)
    args = dict(ray_num=96, coarse_pnum=32, fine_pnum=64, seed=1234)
    args.update(kw)
    return TrainStep(prop, net, opt, (24, 32), (30.0, 28.0), near, far, scene=scene, **args)


def test_linear_spacing_changes_nothing():
    from nerf_amd import procedures
    prop, mip = _nets()
    pose = O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda()
    focal = O.fov2focal(0.6911112070083618, (50, 50))
    with torch.no_grad():
        for kw in (dict(seed=3), dict(seed=3, contract=True, ipe=True), dict()):
            outs = []
            for extra in ({}, {"spacing": "linear"}):
                torch.manual_seed(1)
                outs.append(procedures.render_image(mip, prop, pose, 50, focal, 2.0, 6.0, 64, white_bkg=True, render_depth=True, **kw, **extra))
            assert torch.equal(outs[0]["rgb"], outs[1]["rgb"]) and torch.equal(outs[0]["depth_img"], outs[1]["depth_img"])
    images, poses = _scene_stack()
    for scene in (None, (images, poses)):
        res = []
        for extra in ({}, {"spacing": "linear"}):
            prop, mip = _nets(train=True)
            st = _train_step(prop, mip, 2.0, 6.0, scene=scene, distortion=0.01, **extra)
            if scene is None:
                st.set_image(images[0], poses[0])
            for _ in range(3):
                st()
            torch.cuda.synchronize()
            res.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
        assert all(torch.equal(a, b) for a, b in zip(*res)), "scene" if scene is not None else "image"


# ------------------------------------------------------------------------------------------------ 9. the training step
NEAR9, FAR9 = 0.2, 1000.0


def _step9(prop, net, bright=False, **kw):
    images, poses = _scene_stack(lo=0.6) if bright else _scene_stack()
    args = dict(ray_num=1024, coarse_pnum=64, fine_pnum=128, seed=5, spacing="disparity", contract=True)
    args.update(kw)
    return _train_step(prop, net, NEAR9, FAR9, scene=(images, poses), **args)


def test_train_step_disparity_scene_learns():
    """4 views of 32 x 24, 1 024 rays, 64 + 128 samples, (0.2, 1000), contraction and 0.01 L_dist: 12 eager steps are finite and the
    image loss of the last three sums below that of the first three.
    The choices the scenario leaves open, and why.  Block colours in [0.6, 1]: the 'small' networks render an opaque grey 0.5, which for
    colours uniform in [0, 1] already IS the best constant image (loss = the colours' variance, nothing to gain in 12 steps, and the
    batch-to-batch noise of 1 024 of 3 072 pixels is ~2 %); with bright blocks the mean colour is learnable at once, and unlike dark
    blocks it cannot be 'learnt' by letting the density die (black background).  lr = 2e-4: Adam's first steps move every parameter
    by about lr whatever the gradient's size, i.e. a pre-activation by lr (1 + |h|_1) over 128-256 inputs, and the 'small' fine
    densities are O(1e-2): at 5e-4 they all cross zero in the third step and the ReLU keeps them there (seen under BOTH spacings), at
    1e-3 in one (tests/test_gpu_distortion.py)."""
    prop, mip = _nets(train=True)
    st = _step9(prop, mip, bright=True, distortion=0.01, lr=2e-4)
    losses, totals, dists = [], [], []
    for _ in range(12):
        loss, img_loss = st()
        losses.append(float(img_loss)); totals.append(float(loss)); dists.append(float(st.dist_loss))
    print("image losses", ["%.5f" % v for v in losses], "dist", ["%.2e" % v for v in dists])
    assert all(math.isfinite(v) for v in losses + totals + dists) and all(v > 0.0 for v in dists)
    assert sum(losses[-3:]) < sum(losses[:3]), losses


def test_train_step_disparity_replayed_equals_eager():
    res = []
    for graphed in (False, True):
        prop, mip = _nets(train=True)
        st = _step9(prop, mip, distortion=0.01, lr=1e-5)
        if graphed:
            st.capture(warmup=2)
            for _ in range(2):
                st()
        else:
            for _ in range(4):
                st()
        torch.cuda.synchronize()
        assert torch.isfinite(st.loss).item()
        res.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
    worst = max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(*res))
    print("captured vs eager after 4 iterations: largest relative parameter difference %.3e" % worst)
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_train_step_disparity_dist_loss_is_l_dist_on_s():
    """dist_loss == 0.01 DistortionLoss(1.0)(weights, s_f), recomputed from the public ops on the same draw (same kernels, same inputs:
    the two fp32 scalars may differ by the rounding of the scale only)"""
    from nerf_amd import ops
    from nerf_amd.addtional import DistortionLoss, ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import inverseSample
    prop, mip = _nets(train=True)
    st = _step9(prop, mip, distortion=0.01, ray_num=256)
    st()
    torch.cuda.synchronize()
    prop2, mip2 = _nets(train=True)
    images, poses = _scene_stack()
    seed_dev = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    if True:                                                                          # (grad mode on: the networks take the training kernels, like the step)
        _, s_c, _, rays, index = ops.sample_scene_rays(images, poses, st.fx, st.fy, 0.0, 1.0, 256, 64, seed_dev=seed_dev)
        assert torch.equal(index, st.ray_index)
        z_c, pts = ops.warp_depths(s_c, NEAR9, FAR9, rays)
        dens = F.softplus(prop2.forward(pts, contract=True))
        pw = maxBlurFilter(ProposalNetwork.get_weights(dens, z_c, rays[:, 3:]), 0.01)
        u = ops.philox_uniforms((256, 129), seed_dev=seed_dev)
        s_f, _ = inverseSample(pw, s_c, 129, sort=True, u=u)
        z_f = ops.warp_depths(s_f, NEAR9, FAR9)[0][..., :-1].contiguous()
        rgbo = mip2.forward_rays(rays, z_f, 128, contract=True)
        _, weights, _ = NeRF.render(rgbo, z_f, rays[:, 3:])
        want = 0.01 * DistortionLoss(1.0)(weights, s_f).item()
    assert want > 0.0
    gate("TrainStep(spacing='disparity') dist_loss vs 0.01 L_dist(weights, s_f) (rel)", abs(st.dist_loss.item() - want) / want, 1e-6)


def test_refnerf_train_step_disparity_runs():
    prop, _ = _nets(train=True)
    net = _ref_net(train=True)
    st = _step9(prop, net, ray_num=64, coarse_pnum=32, fine_pnum=32, prop_normal=True)
    assert st.is_ref and st.prop_normal and st.warped
    loss, img_loss = st()
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and math.isfinite(float(img_loss))
    assert all(bool(torch.isfinite(p).all()) for p in list(net.parameters()) + list(prop.parameters()))
    images, poses = _scene_stack()
    with pytest.raises(ValueError):
        _train_step(prop, net, 0.0, 6.0, scene=(images, poses), spacing="disparity")
    with pytest.raises(ValueError):
        _train_step(prop, net, 2.0, 6.0, scene=(images, poses), spacing="sqrt")


# ------------------------------------------------------------------------------------------------ 10. parameter gradients
PINNED = ("mip.lin_block1.0.weight", "mip.lin_block1.2.weight", "mip.lin_block2.0.weight", "mip.lin_block2.4.bias", "mip.bottle_neck.0.weight",
          "mip.opacity_head.0.weight", "mip.rgb_layer.0.weight", "mip.rgb_layer.2.weight", "prop.layers.0.weight", "prop.layers.4.weight",
          "prop.layers.8.weight", "prop.layers.8.bias")


def test_parameter_gradients_with_disparity_depths():
    """One training step from the public ops on 48 explicit rays with disparity depths, (0.2, 1000), contracted, against fp64 autograd of the
    specification -- with the tolerances of test_train_step_gradients_with_ipe_and_contraction (the ops are the same; only their depths
    are new)."""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalLoss, ProposalNetwork, getBounds
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import inverseSample
    near, far, n, c_n, f_n = 0.2, 1000.0, 48, 32, 64
    prop, mip = _nets(train=True)
    rays, g = _rays(n, 31)
    tgt = torch.rand(n, 3, generator=g)
    s_c = R.coarse_s(torch.rand(n, c_n, generator=g)).contiguous()
    u_inv = torch.rand(n, f_n + 1, generator=g)
    Rc, Sc = rays.cuda(), s_c.cuda()
    z_c, pts = ops.warp_depths(Sc, near, far, Rc)
    dens = F.softplus(prop.forward(pts, contract=True))
    pw = maxBlurFilter(ProposalNetwork.get_weights(dens, z_c, Rc[:, 3:]), 0.01)
    s_all, below = inverseSample(pw, Sc, f_n + 1, sort=True, u=u_inv)
    z_f = ops.warp_depths(s_all, near, far)[0][..., :-1].contiguous()
    rgbo = mip.forward_rays(Rc, z_f, f_n, contract=True)
    rend, wts, _ = NeRF.render(rgbo, z_f, Rc[:, 3:])
    img = torch.mean((rend - tgt.cuda()) ** 2)
    ploss = ProposalLoss()(getBounds(pw, below), wts.detach())
    (img + ploss).backward()
    have = {"mip." + k: v.grad for k, v in mip.named_parameters()}
    have.update({"prop." + k: v.grad for k, v in prop.named_parameters()})
    args = (W.proposal_state("small"), W.mip_state("small"), rays, s_c, s_all.detach().cpu(), below.cpu(), tgt, near, far)
    img64, pl64, rend64, exact = R.train_step(torch.float64, *args)
    _, _, _, ref32 = R.train_step(torch.float32, *args)
    gate("disparity step: rendered colours vs fp64", max_abs(rend.detach().cpu().double(), rend64), 1e-5)
    gate("disparity step: image loss vs fp64 (rel)", abs(img.item() - img64) / max(1.0, img64), 1e-5)
    gate("disparity step: proposal loss vs fp64 (rel)", abs(ploss.item() - pl64) / max(1.0, abs(pl64)), 2e-4)
    for k in PINNED:
        top = exact[k].abs().max().item()
        hip_err = (have[k].detach().cpu().double() - exact[k]).abs().max().item() / top
        ref_err = (ref32[k].double() - exact[k]).abs().max().item() / top
        gate("disparity step: d/d %s vs fp64 (of the largest entry; fp32 spec %.1e)" % (k, ref_err), hip_err, max(2.0 * ref_err, 2e-5))


def test_warped_resample_at_the_largest_accepted_shape():
    """C = 256, K = 384: 5 C + 4 K + 1280 floats per ray, 64 KiB of dynamic LDS for a workgroup's four rays -- the launch size and the
    kernel's carve-up come from one layout function, and nine rays are two full workgroups plus a ragged one.  Same references as
    test_warped_resample_equals_the_chain_of_ops_and_the_spec."""
    from nerf_amd import ops
    near, far, C, K, n = 2.0, 6.0, 256, 384, 9
    rays, g = _rays(n, 356)
    s_c = R.coarse_s(torch.rand(n, C, generator=g)).contiguous()
    density = torch.randn(n, C, generator=g) * 2.0
    u = torch.rand(n, K, generator=g)
    u[3] = 0.5 + torch.rand(K, generator=g) / 300.0           # ray 3: the rank-sort fallback
    Rc, Sc, Dc, Uc = rays.cuda(), s_c.cuda(), density.cuda(), u.cuda()
    z_f, s_f, below, w_prop = ops.warped_resample(Dc, Sc, Rc, Uc, near, far)
    z_c = ops.warp_depths(Sc, near, far)[0]
    w = ops.max_blur(ops.sigma_to_weights(Dc, z_c, Rc[:, 3:].contiguous(), ops.ACT_RELU), 0.01)
    s_chain, below_chain = ops.inverse_sample(w, Sc, Uc, sort=True)
    z_chain = ops.warp_depths(s_chain, near, far)[0]
    assert _same_bits(w_prop, w) and _same_bits(s_f, s_chain) and torch.equal(below, below_chain) and _same_bits(z_f, z_chain)
    assert bool((s_f[:, 1:] >= s_f[:, :-1]).all())
    w_spec = R.proposal_weights(density, s_c, rays[:, 3:], near, far, softplus=False)
    s_spec, below_spec, _ = R.resample(w_spec, s_c, u, near, far)
    gate("warped_resample s_fine vs CPU spec at C=256 K=384", max_abs(s_f.cpu(), s_spec), 5e-6)
    gate("warped_resample share of differing below at C=256 K=384", float((below.cpu() != below_spec).float().mean()), 0.01)
