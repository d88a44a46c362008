"""Scene sampler on the device (nerf_amd_sample_scene_rays / ops.sample_scene_rays / TrainStep(scene=...)): the draw against a host
restatement in Python integers, the K = 1 identity with the image-mode sampler, window and view subset, uniformity, edge cases, and the
scene-mode training step (V = 1 equals image mode bit for bit; V = 3 replays from a hipGraph with no per-iteration input)."""
import numpy as np
import pytest
import torch

from conftest import gate
from test_gpu_distortion import FAR, NEAR, _nets, _scene

pytestmark = pytest.mark.gpu
FX, FY = 9.5, 11.25
SEED = 0x1234_5678_9ABC_DEF


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def _stack(V, H, W):
    """images[v, c, row, col] = ((v 3 + c) H + row) W + col: a pixel's value names it (exact in fp32 below 2^24); poses: V distinct cameras"""
    from oracle import nerf_oracle as O
    images = torch.arange(V * 3 * H * W, dtype=torch.float32).reshape(V, 3, H, W)
    assert V * 3 * H * W < 2 ** 24
    poses = torch.stack([O.pose_spherical(20.0 + 37.0 * v, -30.0 + 5.0 * v, 4.0 + 0.25 * v)[:3] for v in range(V)]).contiguous()
    return images.cuda(), poses.cuda()


def _host_cells(seed, N, P):
    """cell of ray n = (x P) >> 64 with x = words 0, 1 of Philox(key = seed, counter = (n, 0, 0, 'IX')), in Python integers"""
    from oracle import nerf_oracle as O
    n = np.arange(N, dtype=np.uint64)
    w = O.philox4x32_10((n & np.uint64(0xFFFFFFFF)).astype(np.uint32), (n >> np.uint64(32)).astype(np.uint32), np.uint32(0), np.uint32(0x4958),
                        seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return [(((int(a) << 32) | int(b)) * P) >> 64 for a, b in zip(w[0], w[1])]


def _decode(index, H, W):
    v = torch.div(index, H * W, rounding_mode="floor")
    r = index - v * H * W
    row = torch.div(r, W, rounding_mode="floor")
    return v, row, r - row * W


# ------------------------------------------------------------------------------------------------ 1. the draw
def test_exact_draw():
    """V=3, H=5, W=7 (odd: W//2 != W/2), N=1003, C=6 (neither a multiple of 4).  The depth interval is evaluated in the kernel's own fp32
    arithmetic -- base = near + s res, then base + res -- so that it is rigorous: z = fl(base + u res) with 0 <= u res < res is inside it by
    monotonicity of rounding (the real-number interval could be missed by half an ulp at u = 0)."""
    from nerf_amd import ops
    V, H, W, N, C = 3, 5, 7, 1003, 6
    images, poses = _stack(V, H, W)
    pts, z, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=SEED)
    torch.cuda.synchronize()
    wp = H * W
    want = []
    for cell in _host_cells(SEED, N, V * wp):
        k, r = divmod(cell, wp)
        row, col = divmod(r, W)
        want.append((k * H + row) * W + col)
    want = torch.tensor(want, dtype=torch.int64)
    assert index.dtype == torch.int64 and torch.equal(index.cpu(), want)
    v, row, col = _decode(index, H, W)
    assert torch.equal(rgb, images[v, :, row, col])
    coords = torch.stack((col - W // 2, H // 2 - row), -1).contiguous()
    seen = 0
    for vi in range(V):
        m = v == vi
        seen += int(m.sum())
        assert int(m.sum()) > 0
        assert torch.equal(rays[m], ops.pixel_rays(coords[m].contiguous(), poses[vi], FX, FY)), vi
    assert seen == N
    res = torch.tensor((FAR - NEAR) / C, dtype=torch.float32, device="cuda")
    base = torch.tensor(NEAR, dtype=torch.float32, device="cuda") + torch.arange(C, dtype=torch.float32, device="cuda") * res
    assert bool((z >= base).all()) and bool((z <= base + res).all())
    o, d = rays[:, None, :3].double(), rays[:, None, 3:].double()
    dz = d * z[..., None].double()
    err = (pts.double() - (o + dz)).abs() - 2.0 ** -23 * (o.abs() + dz.abs())
    gate("scene sampler pts - (o + d z)_fp64 beyond 2^-23 (|o| + |d z|)", max(0.0, err.max().item()), 0.0)


# ------------------------------------------------------------------------------------------------ 2. K = 1 is image mode
@pytest.mark.parametrize("hw", [(5, 7), (6, 10)])
@pytest.mark.parametrize("crop", [(1., 1.), (0.5, 0.5)])
def test_one_view_is_image_mode(hw, crop):
    from nerf_amd import ops
    from nerf_amd.utils import crop_window, randomFromOneImage
    H, W = hw
    N, C = 1003, 6
    images, poses = _stack(1, H, W)
    seed_dev = torch.full((1,), SEED, dtype=torch.int64, device="cuda")
    pixels, coords = randomFromOneImage(images[0], crop)
    want = ops.sample_training_rays_dev(pixels, coords, poses[0], FX, FY, NEAR, FAR, N, C, seed_dev)
    got = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed_dev=seed_dev, window=crop_window(H, W, crop))
    torch.cuda.synchronize()
    for name, a, b in zip(("pts", "lengths", "rgb", "rays"), got[:4], want):
        assert torch.equal(a, b), name
    if crop == (1., 1.):                                     # and the window defaults to the whole image
        again = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed_dev=seed_dev)
        assert all(torch.equal(a, b) for a, b in zip(again[:4], want))


# ------------------------------------------------------------------------------------------------ 3. window and view subset
def test_window_and_view_subset():
    from nerf_amd import ops
    from nerf_amd.utils import crop_window
    V, H, W, N = 4, 6, 10, 1 << 14
    images, poses = _stack(V, H, W)
    win = crop_window(H, W, (0.5, 0.5))
    assert win == (2, 7, 1, 4)
    for ids in ([3, 1], torch.tensor([3, 1]), torch.tensor([3, 1], device="cuda")):
        _, _, rgb, _, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 0, seed=7, window=win, view_ids=ids)
        v, row, col = _decode(index, H, W)
        assert bool(((v == 3) | (v == 1)).all())
        assert bool(((col >= 2) & (col <= 6) & (row >= 1) & (row <= 3)).all())
        assert torch.unique(index).numel() == 30
        assert torch.equal(rgb, images[v, :, row, col])
    # slot k of the draw is view_ids[k]: the subset [3, 1] is the draw of [0, 1] with the views renamed
    _, _, _, _, i01 = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 0, seed=7, window=win, view_ids=[0, 1])
    v01, row01, col01 = _decode(i01, H, W)
    assert torch.equal(torch.where(v01 == 0, 3, 1), v) and torch.equal(row01, row) and torch.equal(col01, col)
    # a 1 x 1 window: one pixel for every ray of a view
    _, _, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, 1001, 0, seed=7, window=(4, 5, 2, 3), view_ids=[2])
    assert bool((index == (2 * H + 2) * W + 4).all()) and bool((rgb == images[2, :, 2, 4]).all()) and bool((rays == rays[0]).all())
    _, _, _, _, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, 1001, 0, seed=7, window=(4, 5, 2, 3))
    v, row, col = _decode(index, H, W)
    assert bool((row == 2).all()) and bool((col == 4).all()) and torch.unique(v).numel() == V


# ------------------------------------------------------------------------------------------------ 4. uniformity
@pytest.mark.parametrize("seed", [1, 20240229, 2 ** 61 + 17])
def test_uniform_over_cells_and_views(seed):
    """chi-square of the counts over the 180 cells (and over the 3 views) below the 1 - 1e-9 quantile: a correct sampler fails with
    probability ~1e-9 per statistic"""
    from scipy.stats import chi2
    from nerf_amd import ops
    V, H, W, N = 3, 6, 10, 1 << 16
    images, poses = _stack(V, H, W)
    _, _, _, _, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 0, seed=seed)
    cells = torch.bincount(index, minlength=V * H * W).double().cpu()
    assert cells.numel() == V * H * W
    e = N / cells.numel()
    gate("scene sampler chi-square over 180 cells, seed %d" % seed, float(((cells - e) ** 2 / e).sum()), float(chi2.ppf(1.0 - 1e-9, cells.numel() - 1)))
    views = cells.reshape(V, -1).sum(1)
    e = N / V
    gate("scene sampler chi-square over 3 views, seed %d" % seed, float(((views - e) ** 2 / e).sum()), float(chi2.ppf(1.0 - 1e-9, V - 1)))


# ------------------------------------------------------------------------------------------------ 5. edges
def test_edges():
    from nerf_amd import ops
    V, H, W, N, C = 3, 5, 7, 203, 6
    images, poses = _stack(V, H, W)
    full = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=5)
    for kw, c in ((dict(want_samples=False), C), ({}, 0)):
        pts, z, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, c, seed=5, **kw)
        assert pts is None and z is None
        assert torch.equal(rgb, full[2]) and torch.equal(rays, full[3]) and torch.equal(index, full[4])
    assert ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=5, want_index=False)[4] is None
    pts, z, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, 0, C, seed=5)
    assert tuple(pts.shape) == (0, C, 3) and tuple(z.shape) == (0, C) and tuple(rgb.shape) == (0, 3) and tuple(rays.shape) == (0, 6)
    assert tuple(index.shape) == (0,) and index.dtype == torch.int64
    again = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=5)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    seed_dev = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    a = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed_dev=seed_dev)
    assert all(torch.equal(x, y) for x, y in zip(a, full))                    # the device seed is the host seed's key
    ops.advance_seed(seed_dev)
    b = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed_dev=seed_dev)
    assert not torch.equal(a[4], b[4]) and not torch.equal(a[1], b[1])
    keep = torch.zeros(N, dtype=torch.int64, device="cuda")
    out = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=5, index_out=keep)
    assert out[4] is keep and torch.equal(keep, full[4])
    for bad in ([0, 3], [-1], torch.tensor([1, 7]), []):
        with pytest.raises(ValueError):
            ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=5, view_ids=bad)
    with pytest.raises(ValueError):
        ops.sample_scene_rays(images.double(), poses, FX, FY, NEAR, FAR, N, C)
    with pytest.raises(ValueError):
        ops.sample_scene_rays(images[:, :, :, 1:], poses, FX, FY, NEAR, FAR, N, C)
    with pytest.raises(ValueError):
        ops.sample_scene_rays(images, poses[:2], FX, FY, NEAR, FAR, N, C)
    with pytest.raises(Exception, match="window"):
        ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, window=(0, W + 1, 0, H))


def test_scene_sampler_of_utils_takes_its_seed_from_the_cpu_generator():
    from nerf_amd import ops
    from nerf_amd.utils import crop_window, sceneSampler
    V, H, W = 3, 6, 10
    images, poses = _stack(V, H, W)
    torch.manual_seed(11)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(11)
    got = sceneSampler(images, poses, 101, 6, (FY, FX), NEAR, FAR, crop_xy=(0.5, 0.5), view_ids=[2, 0])
    want = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, 101, 6, seed=seed, window=crop_window(H, W, (0.5, 0.5)), view_ids=[2, 0])
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want[:4]))
    torch.manual_seed(11)
    rgb, rays = sceneSampler(images, poses, 101, 6, (FY, FX), NEAR, FAR, crop_xy=(0.5, 0.5), view_ids=[2, 0], output_samples=False)
    assert torch.equal(rgb, want[2]) and torch.equal(rays, want[3])


# ------------------------------------------------------------------------------------------------ 6. TrainStep, V = 1
def _train_step(prop, net, scene=None, lr=1e-3, **kw):
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    img, pose, focal = _scene()
    opt = Adam(list(net.parameters()) + list(prop.parameters()), lr=lr, lr_on_device=True)
    args = dict(ray_num=96, coarse_pnum=32, fine_pnum=64, seed=1234)
    args.update(kw)
    if scene == "one":
        return TrainStep(prop, net, opt, (40, 40), focal, NEAR, FAR, scene=(img[None].contiguous(), pose[None].contiguous()), **args)
    if scene is not None:
        return TrainStep(prop, net, opt, (40, 40), focal, NEAR, FAR, scene=scene, **args)
    st = TrainStep(prop, net, opt, (40, 40), focal, NEAR, FAR, **args)
    st.set_image(img, pose)
    return st


@pytest.mark.parametrize("crop", [(1., 1.), (0.5, 0.5)])
def test_train_step_scene_of_one_view_is_the_image_step(crop):
    """MipNeRF branch: after 3 iterations every parameter is bit-identical to the image-mode step on the same image and pose"""
    out = []
    for scene in (None, "one"):
        prop, mip = _nets()
        st = _train_step(prop, mip, scene=scene, crop_xy=crop)
        assert (st.image is None) == (scene is not None)
        for _ in range(3):
            st()
        torch.cuda.synchronize()
        out.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
        assert torch.isfinite(st.loss).item()
    assert all(torch.equal(a, b) for a, b in zip(*out))
    v, row, col = _decode(st.ray_index, 40, 40)
    assert bool((v == 0).all()) and st.ray_index.dtype == torch.int64 and tuple(st.ray_index.shape) == (96,)
    if crop != (1., 1.):
        assert bool(((row >= 10) & (row < 30) & (col >= 10) & (col < 30)).all())


def test_refnerf_train_step_scene_of_one_view_is_the_image_step():
    """Ref-NeRF branch with prop_normal, one iteration: loss and img_loss of the scene-mode step against the image-mode step, within the
    spread between two image-mode runs from the same state.  That spread is printed; on the MI355X it measured 0 (both runs 7.11579418 /
    0.135150105: the step is repeatable), so the check is equality, and scene mode gave the same two numbers."""
    import weights as W
    from nerf_amd.ref_model import RefNeRF
    res = []
    for scene in (None, None, "one"):
        prop, _ = _nets()
        net = RefNeRF(10, 4)
        net.load_state_dict(W.ref_state("small"))
        net = net.cuda().train()
        st = _train_step(prop, net, scene=scene, lr=5e-4, ray_num=64, coarse_pnum=32, fine_pnum=32, seed=31, prop_normal=True)
        loss, img_loss = st()
        res.append((float(loss.item()), float(img_loss.item())))
        st.release()
    (la, ia), (lb, ib), (ls, is_) = res
    print("Ref-NeRF image-mode step twice: loss %.9g / %.9g  img_loss %.9g / %.9g; scene mode: %.9g / %.9g" % (la, lb, ia, ib, ls, is_))
    assert la == la and abs(la) < 1e3
    gate("Ref-NeRF scene-mode loss vs image mode beyond the image-mode run-to-run spread", max(0.0, abs(ls - la) - abs(la - lb)), 0.0)
    gate("Ref-NeRF scene-mode img_loss vs image mode beyond the image-mode run-to-run spread", max(0.0, abs(is_ - ia) - abs(ia - ib)), 0.0)


# ------------------------------------------------------------------------------------------------ 7. TrainStep, V = 3, captured
def _scene3():
    from oracle import nerf_oracle as O
    gen = torch.Generator().manual_seed(17)
    images = torch.rand(3, 3, 40, 40, generator=gen).cuda()
    poses = torch.stack([O.pose_spherical(20.0 + 40.0 * v, -30.0, 4.0)[:3] for v in range(3)]).contiguous().cuda()
    return images, poses


def test_train_step_scene_replayed_equals_eager():
    images, poses = _scene3()
    res = []
    for graphed in (False, True):
        prop, mip = _nets()
        st = _train_step(prop, mip, scene=(images, poses), lr=1e-5)          # (lr as in test_train_step_distortion_replayed_equals_eager)
        if graphed:
            st.capture(warmup=2)
            drawn = []
            for _ in range(4):
                st()                                                         # no argument: the step has no per-iteration input
                drawn.append(st.ray_index.clone())
            torch.cuda.synchronize()
            assert all(not torch.equal(a, b) for a, b in zip(drawn, drawn[1:]))
            assert torch.unique(_decode(torch.cat(drawn), 40, 40)[0]).numel() > 1
            assert bool((torch.cat(drawn) >= 0).all()) and bool((torch.cat(drawn) < 3 * 40 * 40).all())
        else:
            for _ in range(6):
                st()
        torch.cuda.synchronize()
        assert torch.isfinite(st.loss).item()
        res.append([p.detach().clone() for p in list(mip.parameters()) + list(prop.parameters())])
    for a, b in zip(res[1], res[0]):
        assert (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())
    with pytest.raises(ValueError):
        st.set_image(images[0], poses[0])
    with pytest.raises(ValueError):
        st(images[0], poses[0])
    st.set_crop((0.5, 0.5))
    assert st.graph is None
    st.capture(warmup=1)
    st()
    torch.cuda.synchronize()
    _, row, col = _decode(st.ray_index, 40, 40)
    assert bool(((row >= 10) & (row < 30) & (col >= 10) & (col < 30)).all()) and torch.isfinite(st.loss).item()


def test_train_step_scene_arguments():
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    images, poses = _scene3()
    prop, mip = _nets()
    _, _, focal = _scene()
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=1e-3, lr_on_device=True)
    with pytest.raises(ValueError, match="image_hw"):
        TrainStep(prop, mip, opt, (40, 41), focal, NEAR, FAR, scene=(images, poses))
    with pytest.raises(ValueError):
        TrainStep(prop, mip, opt, (40, 40), focal, NEAR, FAR, scene=(images, poses[:2]))
    with pytest.raises(ValueError):
        TrainStep(prop, mip, opt, (40, 40), focal, NEAR, FAR, scene=(images, poses), view_ids=[3])
    with pytest.raises(ValueError):
        TrainStep(prop, mip, opt, (40, 40), focal, NEAR, FAR, view_ids=[0])
    st = TrainStep(prop, mip, opt, (40, 40), focal, NEAR, FAR, ray_num=96, coarse_pnum=32, fine_pnum=64, seed=3, scene=(images, poses), view_ids=[2])
    st()
    torch.cuda.synchronize()
    assert bool((_decode(st.ray_index, 40, 40)[0] == 2).all()) and st.scene[0] is images and st.scene[1] is poses
