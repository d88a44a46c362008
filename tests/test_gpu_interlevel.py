"""Interlevel loss on the device (nerf_amd_interlevel_loss[_backward]) against the fp64 specification of tests/interlevel_ref.py -- loss,
gradient and the bounds, closed and open form, with and without exact edge ties --, exact cases, determinism, and the two users:
TrainStep(prop_loss="interlevel", prop_rounds=...) and render_image(prop_rounds=2)."""
import pytest
import torch
import torch.nn.functional as F

import interlevel_ref as R
from conftest import gate
from test_gpu_distortion import NEAR, FAR, _nets, _rel, _scene, _step, l_dist_spec

pytestmark = pytest.mark.gpu
NS = (1, 63, 65, 4097)
VARIANTS = [(o, t) for o in (False, True) for t in (False, True)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def _hip(w, t, w_prop, t_prop, scale=1.0):
    """-> (loss, d loss / d w_prop, bounds) of the kernels, through InterlevelLoss and ops.interlevel_loss(want_bounds=True)"""
    from nerf_amd import ops
    from nerf_amd.addtional import InterlevelLoss
    w, t, w_prop, t_prop = (x.cuda() for x in (w, t, w_prop, t_prop))
    p = w_prop.clone().requires_grad_(True)
    loss = InterlevelLoss(scale)(w, t, p, t_prop)
    grad, = torch.autograd.grad(loss, p)
    loss2, bounds = ops.interlevel_loss(w, t, w_prop, t_prop, scale, want_bounds=True)
    assert torch.equal(loss2, loss.detach())
    return loss.detach(), grad, bounds


def _errors(x, scale=1.0):
    """(loss rel, gradient of its largest entry, bounds of the largest bound in units of 2^-23) against fp64 evaluated on the device"""
    loss, grad, bounds = _hip(*x, scale=scale)
    b64, l64, g64 = R.evaluate(*(v.cuda() for v in x), scale=scale)
    e_l = abs(loss.item() - l64) / abs(l64) if l64 != 0.0 else abs(loss.item())
    e_g = _rel(grad, g64) if g64.abs().max().item() > 0.0 else grad.abs().max().item()
    e_b = ((bounds.double() - b64).abs().max() / b64.abs().max().clamp_min(1e-300)).item() * 2.0 ** 23
    return e_l, e_g, e_b


@pytest.mark.parametrize("N", NS)
def test_sweep_against_fp64(N):
    """every (M, K) of the list -- one interval, ragged against the 64 lanes, the two-wave workgroups of the longest rows --, closed and
    open, with and without ties.  fp64 accumulation leaves the fp32 rounding of the stored value, 6e-8: the gates are 1e-6 (loss, relative;
    gradient, of its largest entry) and one ulp of the largest bound for bounds_out."""
    worst = [0.0, 0.0, 0.0]
    for M, K in R.GPU_SHAPES:
        for open_form, ties in VARIANTS:
            e = _errors(R.make_inputs(N, M, K, open_form, ties, 1000 * N + 10 * M + K), scale=0.5 if M == 64 else 1.0)
            worst = [max(a, b) for a, b in zip(worst, e)]
            assert worst[0] <= 1e-6 and worst[1] <= 1e-6 and worst[2] <= 1.0, (N, M, K, open_form, ties, e)
    gate("interlevel sweep N=%d loss vs fp64 (rel)" % N, worst[0], 1e-6)
    gate("interlevel sweep N=%d d/dw_prop vs fp64 (of the largest entry)" % N, worst[1], 1e-6)
    gate("interlevel sweep N=%d bounds vs fp64 (of the largest bound, in 2^-23)" % N, worst[2], 1.0)


def test_the_training_shape_against_fp64():
    e = _errors(R.make_inputs(1 << 14, 128, 64, True, False, 77))
    gate("interlevel 2^14 x 128 x 64 loss vs fp64 (rel)", e[0], 1e-6)
    gate("interlevel 2^14 x 128 x 64 d/dw_prop vs fp64 (of the largest entry)", e[1], 1e-6)
    gate("interlevel 2^14 x 128 x 64 bounds vs fp64 (of the largest bound, in 2^-23)", e[2], 1.0)


# ------------------------------------------------------------------------------------------------ exact cases
def test_identical_histograms_give_exactly_zero():
    w, t, _, _ = R.make_inputs(65, 63, 63, False, False, 11)
    loss, grad, bounds = _hip(w, t, w, t)
    assert loss.item() == 0.0 and torch.equal(grad, torch.zeros_like(grad))
    assert bool((bounds >= w.cuda()).all())


def test_fine_rows_outside_a_closed_proposal_span():
    """entirely below and entirely above: every bound 0, the loss sum w^2 / (w + 1e-8), no gradient"""
    w, t, w_prop, t_prop = R.make_inputs(66, 65, 63, False, False, 12)
    t = torch.cat((t[:33] - 10.0, t[33:] + 10.0))
    loss, grad, bounds = _hip(w, t, w_prop, t_prop)
    want = (w.double() ** 2 / (w.double() + 1e-8)).sum().item()
    assert torch.equal(bounds, torch.zeros_like(bounds)) and torch.equal(grad, torch.zeros_like(grad))
    assert abs(loss.item() - want) <= 1e-6 * want


def test_open_form_past_the_last_depth_is_bounded_by_the_last_weight():
    w, t, w_prop, t_prop = R.make_inputs(65, 64, 33, True, False, 13)
    t = t + 10.0                                                                     # every fine edge is past the last proposal depth
    loss, grad, bounds = _hip(w, t, w_prop, t_prop)
    assert torch.equal(bounds, w_prop[:, -1:].cuda().expand_as(bounds))
    assert bool((grad[:, :-1] == 0).all()) and bool((grad[:, -1] < 0).any())
    b64, l64, g64 = R.evaluate(w, t, w_prop, t_prop)
    assert abs(loss.item() - l64) <= 1e-6 * l64 and _rel(grad.cpu(), g64) <= 1e-6


def test_zero_proposal_weights():
    w, t, w_prop, t_prop = R.make_inputs(65, 64, 33, False, True, 14)
    w_prop = torch.zeros_like(w_prop)
    loss, grad, bounds = _hip(w, t, w_prop, t_prop)
    b64, l64, g64 = R.evaluate(w, t, w_prop, t_prop)
    assert torch.equal(bounds, torch.zeros_like(bounds))
    assert abs(loss.item() - l64) <= 1e-6 * l64 and _rel(grad.cpu(), g64) <= 1e-6 and bool((g64 != 0).any())


# ------------------------------------------------------------------------------------------------ other kernel checks
def test_determinism():
    x = R.make_inputs(4097, 128, 64, True, True, 7)
    a, b = _hip(*x), _hip(*x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_only_the_requested_outputs_are_written():
    """bounds_out = NULL leaves a poisoned buffer alone (the C-ABI called directly on it and its neighbours); the backward writes d_w_prop
    and nothing around it"""
    import ctypes as C
    from nerf_amd import ops
    from nerf_amd._lib import lib
    N, M, K = 65, 63, 65
    w, t, w_prop, t_prop = (x.cuda() for x in R.make_inputs(N, M, K, False, False, 15))
    ptr = lambda x: C.c_void_p(x.data_ptr())                                         # noqa: E731
    arena = torch.full((3 * N * M,), -7.0, device="cuda")                             # [guard | what bounds_out would be | guard]
    out = torch.full((3,), -7.0, device="cuda")
    ws = torch.empty(ops.INTERLEVEL_WORKSPACE_FLOATS, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.nerf_amd_interlevel_loss(ptr(w), ptr(t), ptr(w_prop), ptr(t_prop), N, M, K, K + 1, 1.0, ptr(out[1:]), None, ptr(ws), stream) == 0
    torch.cuda.synchronize()
    assert bool((arena == -7.0).all()) and out[0].item() == -7.0 and out[2].item() == -7.0 and out[1].item() > 0.0
    assert lib.nerf_amd_interlevel_loss(ptr(w), ptr(t), ptr(w_prop), ptr(t_prop), N, M, K, K + 1, 1.0, ptr(out[1:]), ptr(arena[N * M:]), ptr(ws),
                                        stream) == 0
    torch.cuda.synchronize()
    assert bool((arena[:N * M] == -7.0).all()) and bool((arena[2 * N * M:] == -7.0).all()) and bool((arena[N * M: 2 * N * M] != -7.0).all())
    grads = torch.full((3 * N * K,), -7.0, device="cuda")
    g = torch.ones(1, device="cuda")
    before = [x.clone() for x in (w, t, w_prop, t_prop)]
    assert lib.nerf_amd_interlevel_loss_backward(ptr(w), ptr(t), ptr(w_prop), ptr(t_prop), N, M, K, K + 1, 1.0, ptr(g), ptr(grads[N * K:]), stream) == 0
    torch.cuda.synchronize()
    assert bool((grads[:N * K] == -7.0).all()) and bool((grads[2 * N * K:] == -7.0).all()) and bool((grads[N * K: 2 * N * K] != -7.0).all())
    assert all(torch.equal(a, b) for a, b in zip(before, (w, t, w_prop, t_prop)))
    assert torch.equal(grads[N * K: 2 * N * K].view(N, K), ops.interlevel_loss_backward(g, w, t, w_prop, t_prop, 1.0))


def test_rows_above_the_limit_are_refused_at_forward_time():
    from nerf_amd.addtional import InterlevelLoss
    for M, K in ((1025, 64), (64, 1025)):
        w, t, w_prop, t_prop = (x.cuda() for x in R.make_inputs(2, M, K, True, False, 1))
        with pytest.raises(NotImplementedError):
            InterlevelLoss()(w, t, w_prop.requires_grad_(True), t_prop)
        with pytest.raises(NotImplementedError):
            InterlevelLoss()(w, t, w_prop.detach(), t_prop)


def test_refnerf_combinations_raise():
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.procedures import render_image
    from nerf_amd.ref_model import RefNeRF
    for kw in (dict(prop_loss="interlevel"), dict(prop_loss="interlevel", prop_rounds=2)):
        with pytest.raises(NotImplementedError):
            _step(ProposalNetwork(10, 256).cuda(), RefNeRF(10, 4).cuda(), **kw)
    prop, mip = _nets()
    with pytest.raises(ValueError):
        _step(prop, mip, prop_rounds=2)                                              # the second round needs the interlevel loss
    with pytest.raises(ValueError):
        _step(prop, mip, prop_loss="overlap")
    img, pose, focal = _scene()
    with pytest.raises(NotImplementedError):
        render_image(RefNeRF(10, 4).cuda(), prop, pose, 40, focal, NEAR, FAR, 64, prop_rounds=2)


# ------------------------------------------------------------------------------------------------ TrainStep
LAM = 0.05
FULL = dict(contract=True, spacing="disparity", distortion=LAM)


def _iteration(prop, mip, img, pose, focal, N, C, P, Fn, seed, rounds, full):
    """TrainStep's MipNeRF-branch forward written out from public ops on the same device-resident random streams -> rendered, target,
    fine weights, fine edges (s under disparity spacing) and the proposal histograms [(w1, e1)(, (w2, e2))]; `full` = contraction +
    disparity spacing"""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import _focal_xy, inverseSample, randomFromOneImage
    fx, fy = _focal_xy(focal)
    seed_dev = torch.full((1,), seed, dtype=torch.int64, device="cuda")
    pixels, coords = randomFromOneImage(img, (1.0, 1.0))
    near, far = (0.0, 1.0) if full else (NEAR, FAR)
    pts, e, rgb_tgt, rays = ops.sample_training_rays_dev(pixels, coords, pose, fx, fy, near, far, N, C, seed_dev)
    dirs = rays[:, 3:]

    def histogram(e, pts):
        z = e
        if full:
            z, pts = ops.warp_depths(e, NEAR, FAR, rays)
        elif pts is None:
            pts = NeRF.length2pts(rays, e)[..., :3].contiguous()
        density = F.softplus(prop.forward(pts, contract=True) if full else prop.forward(pts))
        return maxBlurFilter(ProposalNetwork.get_weights(density, z, dirs), 0.01)

    hists = [(histogram(e, pts), e)]
    if rounds == 2:
        u12 = ops.philox_uniforms((N, P + Fn + 1), seed_dev=seed_dev)
        u = u12[:, P:].contiguous()
        e = inverseSample(hists[0][0], e, P, sort=True, u=u12[:, :P].contiguous())[0]
        hists.append((histogram(e, None), e))
    else:
        u = ops.philox_uniforms((N, Fn + 1), seed_dev=seed_dev)
    edges = inverseSample(hists[-1][0], e, Fn + 1, sort=True, u=u)[0]
    z_f = (ops.warp_depths(edges, NEAR, FAR)[0] if full else edges)[..., :-1].contiguous()
    rgbo = mip.forward_rays(rays, z_f, Fn, contract=True) if full else mip.forward(NeRF.length2pts(rays, z_f))
    rendered, weights, _ = NeRF.render(rgbo, z_f, dirs)
    return rendered, rgb_tgt, weights, edges, hists


def _l_prop64(weights, edges, hists):
    """the interlevel term(s) as the fp64 specification, differentiable in the proposal weights"""
    w, t = weights.detach().double(), edges.detach().double()
    return sum(R.loss_from_bounds(w, R.spec_bounds(t, p.double(), e.detach().double())) for p, e in hists)


@pytest.mark.parametrize("full", [False, True], ids=["plain", "contract-disparity-distortion"])
@pytest.mark.parametrize("rounds", [1, 2])
def test_train_step_equals_the_written_out_iteration(rounds, full):
    """one iteration of TrainStep(prop_loss="interlevel", prop_rounds=rounds, flat_grads=False) == the same iteration from public ops on
    the same device seed, the loss term as the fp64 specification whose autograd feeds the HIP backward: the loss, the term and every
    parameter gradient (the gates of test_train_step_with_distortion_equals_the_written_out_iteration)"""
    N, C, P, Fn, seed = 96, 32, 32, 64, 1234
    tag = "TrainStep(interlevel, rounds=%d, %s)" % (rounds, "full" if full else "plain")
    prop, mip = _nets()
    st = _step(prop, mip, flat_grads=False, prop_loss="interlevel", prop_rounds=rounds, prop_pnum=P, **(FULL if full else {}))
    loss_hip, _ = st()
    torch.cuda.synchronize()
    prop2, mip2 = _nets()
    img, pose, focal = _scene()
    rendered, rgb_tgt, weights, edges, hists = _iteration(prop2, mip2, img, pose, focal, N, C, P, Fn, seed, rounds, full)
    l_prop = _l_prop64(weights, edges, hists)
    img_loss = torch.mean((rendered - rgb_tgt) ** 2)
    loss = l_prop.float() + img_loss
    if full:
        loss = loss + (LAM * l_dist_spec(weights.double(), edges.double())).float()
    loss.backward()
    assert l_prop.item() > 0.0
    gate(tag + " loss vs written-out (rel)", abs(loss_hip.item() - loss.item()) / abs(loss.item()), 1e-6)
    gate(tag + " prop_loss_value vs fp64 spec (rel)", abs(st.prop_loss_value.item() - l_prop.item()) / l_prop.item(), 1e-6)
    worst = 0.0
    for a, b in zip(list(mip.parameters()) + list(prop.parameters()), list(mip2.parameters()) + list(prop2.parameters())):
        worst = max(worst, _rel(a.grad, b.grad))
    gate(tag + " gradients vs written-out (of the largest entry)", worst, 1e-5)


def test_train_step_defaults_are_the_step_without_the_keywords():
    out = []
    for kw in ({}, dict(prop_loss="reference", prop_rounds=1, prop_pnum=None)):
        prop, mip = _nets()
        st = _step(prop, mip, **kw)
        for _ in range(3):
            st()
        torch.cuda.synchronize()
        out.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_two_rounds_accumulate_in_flat_gradients_like_autograd():
    """the proposal network runs backward twice per step: FlatGradients overwrites on the first and adds on the second, autograd
    (flat_grads=False) adds the second to the first -- a sum of two fp32 terms either way, so the gradients are equal bit for bit"""
    grads = []
    for kw in ({}, dict(flat_grads=False)):
        prop, mip = _nets()
        st = _step(prop, mip, prop_loss="interlevel", prop_rounds=2, **kw)
        st()
        torch.cuda.synchronize()
        assert (st.flat_grads is None) == bool(kw)
        grads.append([p.grad.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
    assert all(bool((g != 0).any()) for g in grads[0][-10:])                         # (the proposal network's ten tensors)
    for k, (a, b) in enumerate(zip(*grads)):
        assert torch.equal(a, b), (k, (a - b).abs().max().item(), b.abs().max().item())


def test_two_rounds_replayed_equals_eager():
    res = []
    for graphed in (False, True):
        prop, mip = _nets()
        st = _step(prop, mip, lr=1e-5, prop_loss="interlevel", prop_rounds=2, **FULL)   # (lr 1e-3 can make every density 0 in one Adam step)
        if graphed:
            st.capture(warmup=2)
            for _ in range(3):
                st()
        else:
            for _ in range(5):
                st()
        torch.cuda.synchronize()
        res.append(([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())], st.prop_loss_value.item(), st.loss.item()))
    (pe, ve, le), (pg, vg, lg) = res
    for a, b in zip(pg, pe):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert ve > 0.0 and abs(vg - ve) <= 1e-5 * ve and abs(lg - le) <= 1e-5 * max(1.0, abs(le))


def test_two_rounds_lower_the_interlevel_loss_of_a_probe_batch():
    """150 eager two-round steps from a fixed seed: the probe batch's two-level L_prop ends lower than it started"""
    img, pose, focal = _scene()
    prop, mip = _nets()
    st = _step(prop, mip, ray_num=256, prop_loss="interlevel", prop_rounds=2)

    def probe():
        with torch.no_grad():
            _, _, weights, edges, hists = _iteration(prop, mip, img, pose, focal, 1024, 32, 32, 64, 99, 2, False)
            return _l_prop64(weights, edges, hists).item()

    start = probe()
    for _ in range(150):
        st()
    end = probe()
    print("two-level L_prop of the probe batch: %.6g -> %.6g" % (start, end))
    assert torch.isfinite(st.img_loss).item() and start > 0.0
    assert end < start, (start, end)


# ------------------------------------------------------------------------------------------------ render_image(prop_rounds=2)
def _render_nets():
    prop, mip = _nets()
    return prop.eval(), mip.eval()


@pytest.fixture(scope="module")
def two_round_image():
    """(kwargs, image dict) of the 40 x 40 two-round render the tests below compare against"""
    prop, mip = _render_nets()
    _, pose, focal = _scene()
    kw = dict(white_bkg=True, render_depth=True, seed=77, prop_rounds=2, prop_pnum=48)
    with torch.no_grad():
        from nerf_amd.procedures import render_image
        return kw, render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, **kw)


def test_render_two_rounds_equals_the_written_out_tile_body(two_round_image):
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.procedures import RENDER_COARSE_PNUM
    from nerf_amd.utils import _focal_xy, inverseSample
    kw, img = two_round_image
    prop, mip = _render_nets()
    _, pose, focal = _scene()
    fx, fy = _focal_xy(focal)
    n, P, Fn = 1600, kw["prop_pnum"], 64
    with torch.no_grad():
        rays = ops.generate_rays(pose[:3], 40, 40, fx, fy, pose.device)               # one 40 x 40 tile: tile order is raster order
        dirs = rays[:, 3:]
        z_base = torch.linspace(NEAR, FAR, RENDER_COARSE_PNUM).cuda()
        u1 = ops.philox_stream((n, RENDER_COARSE_PNUM), kw["seed"], 0, strat=True)
        u12 = ops.philox_stream((n, P + Fn + 1), kw["seed"], 0)
        z, pts = ops.stratified_points(rays, z_base, u1, (FAR - NEAR) / Fn)
        w1 = maxBlurFilter(ProposalNetwork.get_weights(prop.forward(pts), z, dirs), 0.01)
        z2, _ = inverseSample(w1, z, P, sort=True, u=u12[:, :P].contiguous())
        w2 = maxBlurFilter(ProposalNetwork.get_weights(prop.forward(NeRF.length2pts(rays, z2)[..., :3].contiguous()), z2, dirs), 0.01)
        fine, _ = inverseSample(w2, z2, Fn + 1, sort=True, u=u12[:, P:].contiguous())
        fine = fine[..., :-1].contiguous()
        rgb, _, extras = NeRF.render(mip.forward(NeRF.length2pts(rays, fine)), fine, dirs, white_bkg=True, density_act=F.relu, render_depth=(NEAR, FAR))
    assert torch.equal(img["rgb"], rgb.view(40, 40, 3).permute(2, 0, 1))
    assert torch.equal(img["depth_img"][0], extras["depth_img"].reshape(40, 40))


def test_render_two_rounds_shards_and_seed_reproduce_the_image(two_round_image):
    from nerf_amd.procedures import render_image
    kw, img = two_round_image
    prop, mip = _render_nets()
    _, pose, focal = _scene()
    with torch.no_grad():
        again = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, **kw)
        parts = [render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, _shard=s, **kw) for s in ((0, 768), (768, 1600))]
        other = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, **dict(kw, seed=78))
        one = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, **dict(kw, prop_rounds=1))
    assert torch.equal(again["rgb"], img["rgb"]) and torch.equal(again["depth_img"], img["depth_img"])
    assert torch.equal(parts[0]["to_image"](torch.cat([p["rgb_rays"] for p in parts]), 3), img["rgb"])
    assert torch.equal(parts[0]["to_image"](torch.cat([p["depth_rays"] for p in parts]).unsqueeze(-1), 1)[0], img["depth_img"][0])
    assert not torch.equal(other["rgb"], img["rgb"]) and not torch.equal(one["rgb"], img["rgb"])


@pytest.mark.parametrize("spacing", ["linear", "disparity"])
def test_render_one_round_is_the_call_without_the_keyword(spacing):
    from nerf_amd.procedures import render_image
    prop, mip = _render_nets()
    _, pose, focal = _scene()
    kw = dict(white_bkg=True, render_depth=True, seed=5, spacing=spacing, contract=spacing == "disparity")
    with torch.no_grad():
        a = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, **kw)
        b = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, prop_rounds=1, prop_pnum=None, **kw)
        c = render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, prop_rounds=2, ipe=True, **kw)     # the second round under every option
    assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["depth_img"], b["depth_img"])
    assert bool(torch.isfinite(c["rgb"]).all()) and bool(torch.isfinite(c["depth_img"]).all()) and not torch.equal(c["rgb"], a["rgb"])


def test_render_two_rounds_take_philox_uniforms_only():
    from nerf_amd.procedures import render_image
    prop, mip = _render_nets()
    _, pose, focal = _scene()
    for rng in ("reference", "device"):
        with pytest.raises(ValueError):
            render_image(mip, prop, pose, 40, focal, NEAR, FAR, 64, rng=rng, prop_rounds=2)
