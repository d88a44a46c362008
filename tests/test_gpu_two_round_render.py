"""The two proposal rounds behind one entry point (nerf_amd_render_rays_rounds, ops.render_rays_rounds) on the GPU.  The specification is
procedures._render_rays_by_calls(prop_rounds=2): the same chain call by call on the same Philox columns, so every comparison is
torch.equal.  render_image(prop_rounds=2) must take the new route for packed networks and keep the call-by-call one for generic ones."""
import functools

import pytest
import torch
import torch.nn.functional as F

import weights as W
from conftest import gate, max_abs
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
SEED = 4711
SPACINGS = {"linear": (2.0, 6.0, False), "disparity": (0.2, 1000.0, True)}       # spacing -> (near, far, contract)
# (prop_pnum, n_fine): one pdf bin | a histogram that is no multiple of 64 | the workload's shape | C > 128: round two's rows are not held in
# registers | K = 201 > 192: a second pass of the three-samples-per-lane search
SHAPES = ((3, 64), (48, 64), (64, 128), (130, 64), (64, 200))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")
    yield
    nerf_amd.set_precision("fp32")


@functools.lru_cache(maxsize=None)
def _nets(hidden=256):
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, hidden)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small", hidden=hidden) if hidden != 256 else W.mip_state("small"))
    return prop.cuda().eval(), mip.cuda().eval()


def _camera(side):
    return O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda(), O.fov2focal(0.6911112070083618, (side, side))


@functools.lru_cache(maxsize=None)
def _rays(side):
    """the side x side camera's rays, raster order (never written to)"""
    from nerf_amd import ops, utils
    pose, focal = _camera(side)
    fx, fy = utils._focal_xy(focal)
    return ops.generate_rays(pose, side, side, fx, fy, pose.device)


def _precision(name):
    import nerf_amd
    from nerf_amd import ops
    nerf_amd.set_precision(name)
    return ops.BF16 if name == "bf16" else ops.F32


def _both(spacing, precision, P, nf, rays, off=0, ipe_radius=None, dir_norm=None, **kw):
    """((rgb, depth, weights) of ops.render_rays_rounds, (rgb, depth) of _render_rays_by_calls(prop_rounds=2)) on the same seed"""
    from nerf_amd import ops, procedures
    near, far, contract = SPACINGS[spacing]
    prec = _precision(precision)
    prop, mip = _nets()
    z_base = torch.linspace(near, far, 64).cuda()
    with torch.no_grad():
        got = ops.render_rays_rounds(prop.packed(prec), mip.packed(prec, wide=ipe_radius is not None), prec, rays, z_base, nf, near, far, True, prop_pnum=P,
                                     seed=SEED, rng_ray_offset=off, spacing=spacing, contract=contract, ipe_radius=ipe_radius, ipe_dir_norm=dir_norm, **kw)
        want = procedures._render_rays_by_calls(mip, prop, rays, z_base, None, None, nf, near, far, True, True, seed=SEED, ray_offset=off, contract=contract,
                                                ipe_radius=ipe_radius, ipe_dir_norm=dir_norm, spacing=spacing, prop_rounds=2, prop_pnum=P)
    return got[:3], want[:2]


def _assert_equal(got, want, what):
    print("%s: rgb %.3e depth %.3e" % (what, max_abs(got[0], want[0]), max_abs(got[1], want[1])))
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all()), what
    assert float(got[0].std()) > 1e-3, what                                        # not a constant image
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what


# ------------------------------------------------------------------------------------------------ entry against specification
@pytest.mark.parametrize("P,nf", SHAPES)
@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_entry_equals_the_call_by_call_route_fp32(spacing, P, nf):
    got, want = _both(spacing, "fp32", P, nf, _rays(40))
    _assert_equal(got, want, "%s fp32 P %d nf %d, 1600 rays" % (spacing, P, nf))


@pytest.mark.parametrize("P,nf", [(48, 64), (64, 128), (130, 64)])
@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_entry_equals_the_call_by_call_route_bf16(spacing, P, nf):
    got, want = _both(spacing, "bf16", P, nf, _rays(40))
    _assert_equal(got, want, "%s bf16 P %d nf %d, 1600 rays" % (spacing, P, nf))


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_ragged_ray_counts(spacing, precision, N):
    """N = 1: one wave of one workgroup; N = 5: a ragged workgroup of the resampling kernels and a ragged tile of the MLP kernels"""
    rays = _rays(40)[800: 800 + N].contiguous()
    for P, nf in ((48, 64), (64, 128)):
        got, want = _both(spacing, precision, P, nf, rays)
        print("%s %s P %d nf %d, %d rays: rgb %.3e depth %.3e" % (spacing, precision, P, nf, N, max_abs(got[0], want[0]), max_abs(got[1], want[1])))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (P, nf)


@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_windowed_draws_are_keyed_by_the_global_ray_index(spacing):
    """10 000 rays with a ray offset: the call-by-call route crosses its chunk boundaries at 4 096 and 8 192, the entry point renders the
    list in one call; and the offset is really read"""
    rays = _rays(100)
    got, want = _both(spacing, "bf16", 64, 128, rays, off=123457)
    _assert_equal(got, want, "%s bf16 P 64 nf 128, 10 000 rays, offset 123457" % spacing)
    other, _ = _both(spacing, "bf16", 64, 128, rays[:64].contiguous(), off=0)
    assert not torch.equal(other[0], got[0][:64])


def test_weights_are_those_of_nerf_render():
    """want_weights: the chain written out from public ops -- the second round's columns cut out of the stream as a tensor"""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import inverseSample
    prec = _precision("fp32")
    prop, mip = _nets()
    rays = _rays(40)
    near, far, P, nf, n = 2.0, 6.0, 48, 64, 1600
    dirs = rays[:, 3:]
    z_base = torch.linspace(near, far, 64).cuda()
    with torch.no_grad():
        rgb, depth, w, _ = ops.render_rays_rounds(prop.packed(prec), mip.packed(prec), prec, rays, z_base, nf, near, far, True, prop_pnum=P, seed=SEED,
                                                  want_weights=True)
        u1 = ops.philox_stream((n, 64), SEED, 0, strat=True, device="cuda")
        u12 = ops.philox_stream((n, P + nf + 1), SEED, 0, device="cuda")
        z, pts = ops.stratified_points(rays, z_base, u1, (far - near) / nf)
        w1 = maxBlurFilter(ProposalNetwork.get_weights(prop.forward(pts), z, dirs), 0.01)
        z2, _ = inverseSample(w1, z, P, sort=True, u=u12[:, :P].contiguous())
        w2 = maxBlurFilter(ProposalNetwork.get_weights(prop.forward(NeRF.length2pts(rays, z2)[..., :3].contiguous()), z2, dirs), 0.01)
        fine, _ = inverseSample(w2, z2, nf + 1, sort=True, u=u12[:, P:].contiguous())
        fine = fine[..., :-1].contiguous()
        want_rgb, want_w, extras = NeRF.render(mip.forward(NeRF.length2pts(rays, fine)), fine, dirs, white_bkg=True, density_act=F.relu, render_depth=(near, far))
    assert w.shape == (n, nf) and float(w.sum()) > 1.0
    assert torch.equal(w, want_w.reshape(n, nf))
    assert torch.equal(rgb, want_rgb.reshape(n, 3)) and torch.equal(depth, extras["depth_img"].reshape(n))


# ------------------------------------------------------------------------------------------------ integrated PE
# Yardstick: the ONE-round fused route against the ONE-round call-by-call route with the integrated PE -- code this entry point does not
# touch -- measured on an MI355X in the same run as the two-round comparison, per spacing (rgb, depth).  Both 0.0: the two routes agree bit
# for bit, so two rounds must too; otherwise the two-round difference is gated at twice the figure recorded here.
IPE_ROUTE_FIGURE = {"linear": (0.0, 0.0), "disparity": (0.0, 0.0)}


@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_integrated_pe_against_the_one_round_yardstick(spacing):
    from nerf_amd import ops, procedures
    near, far, contract = SPACINGS[spacing]
    prec = _precision("fp32")
    prop, mip = _nets()
    rays, nf, radius = _rays(40), 64, 0.002
    z_base = torch.linspace(near, far, 64).cuda()
    norm = ops.dirs_norm(rays)
    with torch.no_grad():
        if spacing == "linear":
            f_rgb, f_d, _, _ = ops.render_rays(prop.packed(prec), mip.packed(prec, wide=True), prec, rays, z_base, None, None, nf, near, far, True,
                                               contract=contract, ipe_radius=radius, seed=SEED, ipe_dir_norm=norm)
        else:
            f_rgb, f_d, _, _ = ops.render_rays_warped(prop.packed(prec), mip.packed(prec, wide=True), prec, rays, None, None, nf, near, far, True,
                                                      contract=contract, ipe_radius=radius, seed=SEED, ipe_dir_norm=norm, spacing=spacing)
        c_rgb, c_d, _ = procedures._render_rays_by_calls(mip, prop, rays, z_base, None, None, nf, near, far, True, True, seed=SEED, contract=contract,
                                                         ipe_radius=radius, ipe_dir_norm=norm, spacing=spacing)
    one = (max_abs(f_rgb, c_rgb), max_abs(f_d, c_d))
    print("integrated PE, %s, one round, fused vs by-calls: rgb %.3e depth %.3e" % (spacing, *one))
    got, want = _both(spacing, "fp32", 48, nf, rays, ipe_radius=radius, dir_norm=norm)
    two = (max_abs(got[0], want[0]), max_abs(got[1], want[1]))
    print("integrated PE, %s, two rounds, entry vs by-calls: rgb %.3e depth %.3e" % (spacing, *two))
    plain, _ = _both(spacing, "fp32", 48, nf, rays)
    assert float((plain[0] - got[0]).abs().max()) > 1e-6                           # the integrated PE is really on
    shard, _ = _both(spacing, "fp32", 48, nf, rays[40:90].contiguous(), off=40, ipe_radius=radius, dir_norm=norm)
    assert torch.equal(shard[0], got[0][40:90])                                    # a shard encodes with the whole list's direction norm
    assert IPE_ROUTE_FIGURE is not None
    figure = IPE_ROUTE_FIGURE[spacing]
    if figure == (0.0, 0.0):
        assert one == (0.0, 0.0)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    else:
        gate("two rounds + IPE, %s: rgb, entry vs by-calls" % spacing, two[0], 2.0 * figure[0])
        gate("two rounds + IPE, %s: depth, entry vs by-calls" % spacing, two[1], 2.0 * figure[1])


# ------------------------------------------------------------------------------------------------ render_image takes the route
class _Reached(Exception):
    pass


@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_render_image_takes_the_entry_point_for_packed_networks(spacing, monkeypatch):
    from nerf_amd import procedures
    near, far, contract = SPACINGS[spacing]
    _precision("fp32")
    prop, mip = _nets()
    pose, focal = _camera(40)
    kw = dict(white_bkg=True, render_depth=True, seed=SEED, prop_rounds=2, prop_pnum=48, spacing=spacing, contract=contract)
    with torch.no_grad():
        want = procedures._render_rays_by_calls(mip, prop, _rays(40), torch.linspace(near, far, 64).cuda(), None, None, 64, near, far, True, True, seed=SEED,
                                                contract=contract, spacing=spacing, prop_rounds=2, prop_pnum=48)

        def refuse(*a, **k):
            raise _Reached()

        monkeypatch.setattr(procedures, "_render_rays_by_calls", refuse)
        img = procedures.render_image(mip, prop, pose, 40, focal, near, far, 64, **kw)
        assert torch.equal(img["rgb"], want[0].view(40, 40, 3).permute(2, 0, 1)) and torch.equal(img["depth_img"][0], want[1].view(40, 40))
        with pytest.raises(_Reached):                                               # a layer-by-layer network keeps the call-by-call route
            procedures.render_image(_nets(320)[1], prop, pose, 40, focal, near, far, 64, **kw)
        with pytest.raises(_Reached):                                               # and so does a histogram size below the entry point's
            procedures.render_image(mip, prop, pose, 40, focal, near, far, 64, **dict(kw, prop_pnum=2))


# ------------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_shards_reproduce_the_image_and_the_seed_matters(spacing):
    from nerf_amd.procedures import render_image
    near, far, contract = SPACINGS[spacing]
    _precision("fp32")
    prop, mip = _nets()
    pose, focal = _camera(40)
    kw = dict(white_bkg=True, render_depth=True, seed=SEED, prop_rounds=2, prop_pnum=64, spacing=spacing, contract=contract)
    with torch.no_grad():
        img = render_image(mip, prop, pose, 40, focal, near, far, 64, **kw)
        parts = [render_image(mip, prop, pose, 40, focal, near, far, 64, _shard=s, **kw) for s in ((0, 777), (777, 1600))]
        other = render_image(mip, prop, pose, 40, focal, near, far, 64, **dict(kw, seed=SEED + 1))
    assert torch.equal(parts[0]["to_image"](torch.cat([p["rgb_rays"] for p in parts]), 3), img["rgb"])
    assert torch.equal(parts[0]["to_image"](torch.cat([p["depth_rays"] for p in parts]).unsqueeze(-1), 1)[0], img["depth_img"][0])
    assert not torch.equal(other["rgb"], img["rgb"])


# ------------------------------------------------------------------------------------------------ workspace
@pytest.mark.parametrize("spacing", list(SPACINGS))
def test_workspace_is_not_overrun_and_an_undersized_one_is_replaced(spacing):
    from nerf_amd import _lib, ops
    near, far, contract = SPACINGS[spacing]
    prec = _precision("fp32")
    prop, mip = _nets()
    rays = _rays(40)[:333].contiguous()
    P, nf = 130, 64
    z_base = torch.linspace(near, far, 64).cuda()
    need = _lib.lib.nerf_amd_render_rounds_workspace_bytes(333, nf, P, _lib.SPACINGS[spacing])
    assert need > 0
    args = (prop.packed(prec), mip.packed(prec), prec, rays, z_base, nf, near, far, True)
    kw = dict(prop_pnum=P, seed=SEED, spacing=spacing, contract=contract)
    guarded = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb, _, _, used = ops.render_rays_rounds(*args, workspace=guarded, **kw)
    torch.cuda.synchronize()
    assert used is guarded
    assert bool((guarded[need:] == 0xA5).all())
    assert not bool((guarded[:need] == 0xA5).all())
    small = torch.full((need - 1,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb2, _, _, used2 = ops.render_rays_rounds(*args, workspace=small, **kw)
    torch.cuda.synchronize()
    assert used2 is not small and used2.numel() >= need
    assert bool((small == 0xA5).all())
    assert torch.equal(rgb, rgb2)
