"""Distortion regularisers on the device (nerf_amd_distortion_loss[_backward]): the reference's Regularizer (addtional.py:26-35, mode 0)
against golden G26 (the real reference in fp32) and an fp64 spec, Mip-NeRF 360's L_dist (DistortionLoss, mode 1) against an fp64 pairwise
spec, determinism, and TrainStep(distortion=...) -- wiring, hipGraph replay, and that the term does what it is for."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 2.0, 6.0
NS = (1, 63, 65, 4097)
SS = (2, 3, 64, 65, 129, 257, 1024)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


# ------------------------------------------------------------------------------------------------ fp64 specifications, chunked over rays
def _part(w, t, mode, N, dtype):
    """the loss of a chunk of rays, normalised by the whole batch's N: mode 0 the reference's expression, mode 1 L_dist.  The centres,
    widths and (mode 0) averaged weights are formed from the fp32 inputs in fp32, as the reference forms them, everything after in
    `dtype`: the depths' gradient is ill-conditioned in the centres where they come close (rows in any order), so the exact-centre value
    differs from the reference's own by up to 8e-5 of its largest entry (S = 1024, unsorted)"""
    M = t.shape[-1] - 1
    c = ((t[..., :-1] + t[..., 1:]) / 2.).to(dtype)
    delta = (t[..., 1:] - t[..., :-1]).to(dtype)
    if mode == 0:
        dists = torch.abs(c[:, None, :] - c[..., None])
        dists = dists / dists.norm(dim=-1, keepdim=True)
        a = ((w[..., :-1] + w[..., 1:]) / 2.).to(dtype)
        return (a[:, None, :] * a[..., None] * dists).sum() / (N * M * M) + (delta * a ** 2).sum() / (3 * N * M)
    w = w.to(dtype)
    pair = (w[:, :, None] * w[:, None, :] * torch.abs(c[:, :, None] - c[:, None, :])).sum()
    return (pair + (w * w * delta).sum() / 3.) / N


def spec(w, t, mode, dtype=torch.float64):
    """-> (loss, d/dw, d/dt) by autograd in `dtype` on fp32 inputs (see _part), in chunks of rays whose (n, M, M) intermediates stay
    below 2^26 elements"""
    w32, t32 = w.detach().float(), t.detach().float()
    N, M = t.shape[0], t.shape[1] - 1
    step = max(1, (1 << 26) // (M * M))
    loss, gw, gt = 0.0, torch.empty_like(w32, dtype=torch.float64), torch.empty_like(t32, dtype=torch.float64)
    for s0 in range(0, N, step):
        ww, tt = w32[s0:s0 + step].clone().requires_grad_(True), t32[s0:s0 + step].clone().requires_grad_(True)
        part = _part(ww, tt, mode, N, dtype)
        gw[s0:s0 + step], gt[s0:s0 + step] = torch.autograd.grad(part, (ww, tt))
        loss += part.item()
    return loss, gw, gt


def _rel(a, b):
    """max |a - b| relative to the largest entry of b"""
    b = b.double()
    return ((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _hip(module, w, t):
    w = w.cuda().requires_grad_(True)
    t = t.cuda().requires_grad_(True)
    loss = module(w, t)
    gw, gt = torch.autograd.grad(loss, (w, t))
    return loss, gw, gt


def _inputs(N, S, mode, seed):
    g = torch.Generator().manual_seed(seed)
    t = 2.0 + 4.0 * torch.rand(N, S, generator=g)
    if mode == 1:
        t = torch.sort(t, dim=-1)[0]
    w = torch.rand(N, S if mode == 0 else S - 1, generator=g)
    return w, t


# ------------------------------------------------------------------------------------------------ Regularizer (mode 0)
@pytest.mark.parametrize("case", ["pipe", "unsort", "nan", "s257"])
def test_regularizer_against_g26_and_fp64(golden, case):
    from nerf_amd.addtional import Regularizer
    g = golden("g26_regularizer")
    w, t = g[case + "_w"], g[case + "_t"]
    loss, gw, gt = _hip(Regularizer(), w, t)
    torch.cuda.synchronize()
    if case == "nan":                                            # one interval per ray: r = 0, the reference's 0/0
        assert torch.isnan(loss).item() and torch.isnan(gw).all().item() and torch.isnan(gt).all().item()
        assert torch.isnan(g[case + "_gw"]).all().item() and torch.isnan(g[case + "_gt"]).all().item()
        return
    want = float(g[case + "_loss"])
    l64, gw64, gt64 = spec(w, t, 0)
    gate("regularizer g26 %s loss vs reference fp32 (rel)" % case, abs(loss.item() - want) / abs(want), 1e-5)
    gate("regularizer g26 %s loss vs fp64 (rel)" % case, abs(loss.item() - l64) / abs(l64), 1e-6)
    gate("regularizer g26 %s d/dw vs reference fp32" % case, _rel(gw.cpu(), g[case + "_gw"]), 1e-5)
    gate("regularizer g26 %s d/dt vs reference fp32" % case, _rel(gt.cpu(), g[case + "_gt"]), 1e-5)
    gate("regularizer g26 %s d/dw vs fp64" % case, _rel(gw.cpu(), gw64), 1e-6)
    gate("regularizer g26 %s d/dt vs fp64" % case, _rel(gt.cpu(), gt64), 1e-6)




def _sweep(mode, module, extra=()):
    """worst errors against fp64 -- loss relative, gradients relative to their largest entry"""
    worst = {"loss": 0.0, "w": 0.0, "t": 0.0}
    for N, S in [(n, s) for n in NS for s in SS] + list(extra):
        w, t = _inputs(N, S, mode, 1000 * N + S)
        loss, gw, gt = _hip(module, w, t)
        l64, gw64, gt64 = spec(w.cuda(), t.cuda(), mode)
        if mode == 0 and S == 2:
            assert torch.isnan(loss).item() and l64 != l64, (N, S)
            continue
        worst["loss"] = max(worst["loss"], abs(loss.item() - l64) / abs(l64))
        worst["w"] = max(worst["w"], _rel(gw, gw64))
        worst["t"] = max(worst["t"], _rel(gt, gt64))
        assert worst["loss"] <= 1e-6 and worst["w"] <= 1e-6 and worst["t"] <= 1e-6, (N, S, worst)
    return worst


def test_regularizer_sweep_against_fp64():
    """unsorted rows, ragged N and S (one interval to 1023): loss and both gradients against the fp64 spec"""
    from nerf_amd.addtional import Regularizer
    worst = _sweep(0, Regularizer())
    gate("regularizer sweep loss vs fp64 (rel)", worst["loss"], 1e-6)
    gate("regularizer sweep d/dw vs fp64", worst["w"], 1e-6)
    gate("regularizer sweep d/dt vs fp64", worst["t"], 1e-6)


def test_distortion_loss_sweep_against_fp64():
    from nerf_amd.addtional import DistortionLoss
    worst = _sweep(1, DistortionLoss(), extra=[(1 << 14, 129)])
    gate("L_dist sweep loss vs fp64 (rel)", worst["loss"], 1e-6)
    gate("L_dist sweep d/dw vs fp64", worst["w"], 1e-6)
    gate("L_dist sweep d/de vs fp64", worst["t"], 1e-6)


def test_rows_above_the_limit_are_refused_at_forward_time():
    from nerf_amd.addtional import DistortionLoss, Regularizer
    w, t = _inputs(4, 1025, 0, 1)
    for module, ww in ((Regularizer(), w), (DistortionLoss(), w[:, :-1])):
        with pytest.raises(NotImplementedError):
            module(ww.cuda().requires_grad_(True), t.cuda())
        with pytest.raises(NotImplementedError):
            module(ww.cuda(), t.cuda())


def test_only_the_requested_gradient_is_written():
    from nerf_amd import ops
    from nerf_amd.addtional import DistortionLoss
    w, t = _inputs(65, 129, 1, 3)
    g = torch.ones((), device="cuda")
    d_w, d_t = ops.distortion_loss_backward(g, w.cuda(), t.cuda(), 1, 1.0, (True, False))
    assert d_t is None and d_w.shape == w.shape
    d_w2, d_t2 = ops.distortion_loss_backward(g, w.cuda(), t.cuda(), 1, 1.0, (False, True))
    assert d_w2 is None and d_t2.shape == t.shape
    _, ew, et = _hip(DistortionLoss(), w, t)
    assert torch.equal(d_w, ew) and torch.equal(d_t2, et)


def test_determinism():
    from nerf_amd.addtional import DistortionLoss, Regularizer
    for mode, module in ((0, Regularizer()), (1, DistortionLoss())):
        w, t = _inputs(4097, 129, mode, 7)
        a = _hip(module, w, t)
        b = _hip(module, w, t)
        for x, y in zip(a, b):
            assert torch.equal(x, y), mode


# ------------------------------------------------------------------------------------------------ TrainStep(distortion=...)
def _nets():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weights as W
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(W.proposal_state("small"))
    mip.load_state_dict(W.mip_state("small"))
    return prop.cuda().train(), mip.cuda().train()


def _scene(seed=3):
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as O                                      # (test infrastructure: pose / focal only)
    gen = torch.Generator().manual_seed(seed)
    img = torch.rand(3, 40, 40, generator=gen).cuda()
    pose = O.pose_spherical(20.0, -30.0, 4.0)[:3].contiguous().cuda()
    return img, pose, O.fov2focal(0.6911112070083618, (40, 40))


def _step(prop, mip, lr=1e-3, **kw):
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    img, pose, focal = _scene()
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=lr, lr_on_device=True)
    args = dict(ray_num=96, coarse_pnum=32, fine_pnum=64, seed=1234)
    args.update(kw)
    st = TrainStep(prop, mip, opt, (40, 40), focal, NEAR, FAR, **args)
    st.set_image(img, pose)
    return st


def l_dist_spec(w, e):
    """L_dist (mean over rays) in torch, differentiable"""
    m = (e[..., :-1] + e[..., 1:]) / 2.
    pair = (w[:, :, None] * w[:, None, :] * torch.abs(m[:, :, None] - m[:, None, :])).sum((-2, -1))
    return torch.mean(pair + (w * w * (e[..., 1:] - e[..., :-1])).sum(-1) / 3.)


def _forward(prop, mip, img, pose, focal, N, C, Fn, seed, ipe_radius=None, contract=False):
    """TrainStep's MipNeRF-branch forward written out from public ops, on the same device-resident random streams"""
    from nerf_amd import ops
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_methods import maxBlurFilter
    from nerf_amd.nerf_base import NeRF
    from nerf_amd.utils import _focal_xy, inverseSample, randomFromOneImage
    fx, fy = _focal_xy(focal)
    seed_dev = torch.full((1,), seed, dtype=torch.int64, device="cuda")
    pixels, coords = randomFromOneImage(img, (1.0, 1.0))
    pts, z_c, rgb_tgt, rays = ops.sample_training_rays_dev(pixels, coords, pose, fx, fy, NEAR, FAR, N, C, seed_dev)
    dirs = rays[:, 3:]
    density = F.softplus(prop.forward(pts, contract=True) if contract else prop.forward(pts))
    prop_w = maxBlurFilter(ProposalNetwork.get_weights(density, z_c, dirs), 0.01)
    u = ops.philox_uniforms((N, Fn + 1), seed_dev=seed_dev)
    edges, below = inverseSample(prop_w, z_c, Fn + 1, sort=True, u=u)
    z_f = edges[..., :-1].contiguous()
    if ipe_radius is not None:
        rgbo = mip.forward_rays(rays, edges, Fn, ipe_radius=ipe_radius, contract=contract)
    else:
        rgbo = mip.forward_rays(rays, z_f, Fn, contract=True) if contract else mip.forward(NeRF.length2pts(rays, z_f))
    rendered, weights, _ = NeRF.render(rgbo, z_f, dirs)
    return rendered, weights, edges, rgb_tgt, prop_w, below


@pytest.mark.parametrize("variant", ["pe", "ipe", "contract"])
def test_train_step_with_distortion_equals_the_written_out_iteration(variant):
    """one iteration of TrainStep(distortion=lam, flat_grads=False) == the same iteration from public ops with the L_dist term as the
    fp64 torch spec in s = (z - near) / (far - near), whose autograd feeds the HIP render backward: loss and every parameter gradient"""
    from nerf_amd.addtional import ProposalLoss, getBounds
    lam, N, C, Fn, seed = 0.05, 96, 32, 64, 1234
    kw = {"ipe": dict(ipe_radius=2.0 / 12 ** 0.5 / 40.0), "contract": dict(contract=True), "pe": {}}[variant]
    prop, mip = _nets()
    st = _step(prop, mip, flat_grads=False, distortion=lam, **kw)
    loss_hip, _ = st()
    torch.cuda.synchronize()
    prop2, mip2 = _nets()
    img, pose, focal = _scene()
    rendered, weights, edges, rgb_tgt, prop_w, below = _forward(prop2, mip2, img, pose, focal, N, C, Fn, seed, **kw)
    dist = lam * l_dist_spec(weights.double(), (edges.double() - NEAR) / (FAR - NEAR))
    img_loss = torch.mean((rendered - rgb_tgt) ** 2)
    loss = ProposalLoss()(getBounds(prop_w, below), weights.detach()) + img_loss + dist.float()
    loss.backward()
    gate("TrainStep(distortion) %s loss vs written-out (rel)" % variant, abs(loss_hip.item() - loss.item()) / abs(loss.item()), 1e-6)
    gate("TrainStep(distortion) %s dist_loss vs fp64 spec (rel)" % variant, abs(st.dist_loss.item() - dist.item()) / dist.item(), 1e-6)
    worst = 0.0
    for a, b in zip(list(mip.parameters()) + list(prop.parameters()), list(mip2.parameters()) + list(prop2.parameters())):
        worst = max(worst, _rel(a.grad, b.grad))
    gate("TrainStep(distortion) %s gradients vs written-out (of the largest entry)" % variant, worst, 1e-5)


def test_train_step_distortion_zero_is_the_plain_step():
    """distortion=0.0 is the step built without the keyword: parameters bit-identical after 3 iterations"""
    out = []
    for kw in ({}, {"distortion": 0.0}):
        prop, mip = _nets()
        st = _step(prop, mip, **kw)
        for _ in range(3):
            st()
        torch.cuda.synchronize()
        out.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
        assert st.dist_loss.item() == 0.0
    assert all(torch.equal(a, b) for a, b in zip(*out))


def test_train_step_distortion_replayed_equals_eager():
    res = []
    for graphed in (False, True):
        prop, mip = _nets()
        st = _step(prop, mip, lr=1e-5, distortion=0.01, contract=True)      # (lr 1e-3 can make every density 0 in one Adam step)
        if graphed:
            st.capture(warmup=2)
            for _ in range(3):
                st()
        else:
            for _ in range(5):
                st()
        torch.cuda.synchronize()
        res.append(([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())], st.dist_loss.item(), st.loss.item()))
    (pe, de, le), (pg, dg, lg) = res
    for a, b in zip(pg, pe):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    assert de > 0.0 and abs(dg - de) <= 1e-5 * de and abs(lg - le) <= 1e-5 * max(1.0, abs(le))


def test_refnerf_train_step_with_distortion_raises():
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.ref_model import RefNeRF
    with pytest.raises(NotImplementedError):
        _step(ProposalNetwork(10, 256).cuda(), RefNeRF(10, 4).cuda(), distortion=0.01)


def test_distortion_lowers_l_dist_of_a_probe_batch():
    """150 eager steps from the same state and seed with lam = 0 and lam = 0.1: the probe batch's L_dist (in s) ends lower with the term"""
    from nerf_amd.addtional import DistortionLoss
    img, pose, focal = _scene()
    ends = {}
    for lam in (0.0, 0.1):
        prop, mip = _nets()
        st = _step(prop, mip, ray_num=256, distortion=lam)
        for _ in range(150):
            st()
        with torch.no_grad():
            _, weights, edges, _, _, _ = _forward(prop, mip, img, pose, focal, 1024, 32, 64, 99)
            ends[lam] = DistortionLoss(1.0 / (FAR - NEAR))(weights, edges).item()
        assert torch.isfinite(st.img_loss).item()
    assert ends[0.1] < ends[0.0], ends
