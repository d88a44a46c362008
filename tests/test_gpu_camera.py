"""The camera model on the device (nerf_amd_generate_rays_camera / nerf_amd_sample_scene_rays_camera, render_image(camera=...),
TrainStep(cameras=...)): Camera.reference reproduces today's rays bit for bit; an off-centre pinhole, the strong OPENCV camera and a
SIMPLE_RADIAL one meet the two bounds of tests/camera_ref.py (backward error through the fp64 forward model; direction against the fp64
rays); the scene sampler keeps its draw; render_image and TrainStep carry the camera through every layer."""
import numpy as np
import pytest
import torch

import camera_ref as R
from conftest import gate
from test_camera_host import POSE_I, pose_general
from test_gpu_distortion import FAR, NEAR, _nets
from test_gpu_scene_sampler import FX, FY, SEED, _decode, _host_cells, _stack

pytestmark = pytest.mark.gpu
H, W = 33, 47


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def _check_rays(name, row, pose, cols, rows, rays, what):
    """both bounds for rays (n, 6) of the pixels under camera `row`: origins bit-equal; with an identity rotation d = (xu, -yu, -1)
    exactly, so the backward check reads the kernel's point; any rotation: the direction check.  -> the worst err / tol"""
    rays = rays.detach().cpu().numpy()
    pose = np.asarray(pose, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(rays[:, :3], np.broadcast_to(pose[:, 3], (rays.shape[0], 3))), name
    worst = R.direction_ratio(pose, row, cols, rows, rays[:, 3:])
    if np.array_equal(pose[:, :3], np.eye(3, dtype=np.float32)):
        assert np.all(rays[:, 5] == -1.0)
        xu, yu = rays[:, 3], -rays[:, 4]
        if np.any(row[4:9] != 0.0):
            worst = max(worst, R.backward_ratio(row, cols, rows, xu, yu))
        else:                                                            # no iteration: the point is the header's fp32 pixel point itself
            xdh, ydh = R.pixel_plane32(row, cols, rows)
            assert np.array_equal(xu.astype(np.float64), xdh) and np.array_equal(yu.astype(np.float64), ydh), name
    gate("camera %s, %s: worst err / tol over both bounds" % (name, what), worst, 1.0)
    return worst


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("hw", [(5, 7), (8, 6)])
def test_reference_camera_is_todays_ray_table(hw):
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    Hh, Ww = hw
    _, poses = _stack(1, Hh, Ww)
    cam = Camera.reference(Hh, Ww, (FY, FX))
    assert torch.equal(ops.generate_camera_rays(poses[0], Hh, Ww, cam, poses.device), ops.generate_rays(poses[0], Hh, Ww, FX, FY, poses.device))
    assert torch.equal(ops.generate_camera_rays(poses[0], Hh, Ww, cam, poses.device, ray_offset=11, n=17),
                       ops.generate_rays(poses[0], Hh, Ww, FX, FY, poses.device, ray_offset=11, n=17))


def test_sampler_reference_cameras_are_todays_scene_sampler():
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    V, Hh, Ww, N, C = 3, 5, 7, 1003, 6
    images, poses = _stack(V, Hh, Ww)
    want = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=SEED)
    cam = Camera.reference(Hh, Ww, (FY, FX), sampler=True)
    for cameras in (cam, [cam] * V, Camera.table([cam] * V, images.device)):
        got = ops.sample_scene_rays(images, poses, 1.0, 1.0, NEAR, FAR, N, C, seed=SEED, cameras=cameras)      # (fx, fy are ignored)
        for name, a, b in zip(("pts", "lengths", "rgb", "rays", "index"), got, want):
            assert torch.equal(a, b), name
    got = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 0, seed=SEED, cameras=cam, want_index=False)
    assert got[0] is None and got[1] is None and got[4] is None and torch.equal(got[3], want[3])


# ------------------------------------------------------------------------------------------------ 2. specification
@pytest.mark.parametrize("name", ["pinhole", "opencv", "simple_radial"])
def test_ray_table_meets_both_bounds(name):
    from nerf_amd import ops
    row = R.cameras(H, W)[name]
    R.admit(row, H, W)
    cam = R.camera_of(row)
    cols, rows = R.grid(H, W)
    for what, pose in (("identity rotation", POSE_I), ("general pose", pose_general())):
        rays = ops.generate_camera_rays(torch.from_numpy(pose), H, W, cam, "cuda")
        _check_rays(name, row, pose, cols, rows, rays, what)
    part = ops.generate_camera_rays(torch.from_numpy(pose), H, W, cam, "cuda", ray_offset=301, n=777)      # a shard: the same bits
    assert torch.equal(part, rays[301: 301 + 777])


def test_negative_control_swapped_tangential_coefficients():
    """the kernel's table against the camera with p1 and p2 swapped: the check must fail"""
    from nerf_amd import ops
    row = R.cameras(H, W)["opencv"]
    wrong = row.copy()
    wrong[7], wrong[8] = row[8], row[7]
    cols, rows = R.grid(H, W)
    rays = ops.generate_camera_rays(torch.from_numpy(pose_general()), H, W, R.camera_of(row), "cuda").cpu().numpy()
    assert R.direction_ratio(pose_general(), row, cols, rows, rays[:, 3:]) <= 1.0
    assert R.direction_ratio(pose_general(), wrong, cols, rows, rays[:, 3:]) > 1.0
    rays = ops.generate_camera_rays(torch.from_numpy(POSE_I), H, W, R.camera_of(row), "cuda").cpu().numpy()
    assert R.backward_ratio(wrong, cols, rows, rays[:, 3], -rays[:, 4]) > 1.0


def _scene_cameras(Hh, Ww):
    c = R.cameras(Hh, Ww)
    rows = [c["opencv"], c["pinhole"], c["simple_radial"]]                       # three different cameras, one undistorted
    for r in rows:
        R.admit(r, Hh, Ww)
    return rows


@pytest.mark.parametrize("rotation", ["identity", "general"])
def test_scene_sampler_with_three_cameras(rotation):
    """V=3, 9 x 11, N=1003, C=6, a window and view_ids=[2, 0]: the draw is the host restatement's, rgb the named pixel, every ray meets
    the bounds for its own view's camera, depths are the existing sampler's bits and points are o + z d"""
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    V, Hh, Ww, N, C = 3, 9, 11, 1003, 6
    images, poses = _stack(V, Hh, Ww)
    if rotation == "identity":
        poses = torch.stack([torch.from_numpy(POSE_I) + torch.tensor([[0, 0, 0, 0.5 * v]] * 3) for v in range(V)]).contiguous().cuda()
    rows = _scene_cameras(Hh, Ww)
    table = Camera.table([R.camera_of(r) for r in rows], images.device)
    worst = 0.0
    for window, ids in ((None, None), ((2, 9, 1, 7), [2, 0])):
        pts, z, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=SEED, window=window, view_ids=ids, cameras=table)
        plain = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, C, seed=SEED, window=window, view_ids=ids)
        torch.cuda.synchronize()
        x0, x1, y0, y1 = (0, Ww, 0, Hh) if window is None else window
        ww, wp = x1 - x0, (x1 - x0) * (y1 - y0)
        views = list(range(V)) if ids is None else ids
        want = []
        for cell in _host_cells(SEED, N, len(views) * wp):
            k, r = divmod(cell, wp)
            wr, wc = divmod(r, ww)
            want.append((views[k] * Hh + y0 + wr) * Ww + x0 + wc)
        assert index.dtype == torch.int64 and torch.equal(index.cpu(), torch.tensor(want, dtype=torch.int64))
        assert torch.equal(index, plain[4]) and torch.equal(rgb, plain[2]) and torch.equal(z, plain[1])
        v, row, col = _decode(index, Hh, Ww)
        assert torch.equal(rgb, images[v, :, row, col])
        for vi in views:
            m = v == vi
            assert int(m.sum()) > 0
            worst = max(worst, _check_rays("view %d" % vi, rows[vi], poses[vi].cpu().numpy(), col[m].cpu().numpy(), row[m].cpu().numpy(), rays[m],
                                           "scene sampler, %s rotation" % rotation))
        o, d = rays[:, None, :3].double(), rays[:, None, 3:].double()
        dz = d * z[..., None].double()
        err = (pts.double() - (o + dz)).abs() - 2.0 ** -23 * (o.abs() + dz.abs())
        gate("camera scene sampler pts - (o + d z)_fp64 beyond 2^-23 (|o| + |d z|)", max(0.0, err.max().item()), 0.0)
    assert worst > 0.0


def test_scene_sampler_bad_device_view_id():
    """a device view id outside [0, V): NaN rays and colours, index -1, nothing read; the other slot is untouched"""
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    V, Hh, Ww, N = 3, 9, 11, 1003
    images, poses = _stack(V, Hh, Ww)
    table = Camera.table([R.camera_of(r) for r in _scene_cameras(Hh, Ww)], images.device)
    for bad in (5, -1):
        ids = torch.tensor([1, bad], dtype=torch.int64, device="cuda")
        pts, z, rgb, rays, index = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 6, seed=SEED, view_ids=ids, cameras=table)
        good = ops.sample_scene_rays(images, poses, FX, FY, NEAR, FAR, N, 6, seed=SEED, view_ids=[1, 0], cameras=table)
        m = index < 0
        assert 0 < int(m.sum()) < N and bool((index[m] == -1).all())
        assert bool(torch.isnan(rays[m]).all()) and bool(torch.isnan(rgb[m]).all()) and bool(torch.isnan(pts[m]).all())
        v, _, _ = _decode(good[4], Hh, Ww)
        assert torch.equal(m, v == 0)
        assert torch.equal(rays[~m], good[3][~m]) and torch.equal(index[~m], good[4][~m]) and torch.equal(z, good[1])


# ------------------------------------------------------------------------------------------------ 3. render_image
def _render_nets(ref=False):
    prop, mip = _nets()
    if ref:
        import weights as Wt
        from nerf_amd.ref_model import RefNeRF
        mip = RefNeRF(10, 4)
        mip.load_state_dict(Wt.ref_state("small"))
        mip = mip.cuda()
    return prop.eval(), mip.eval()


def _pose():
    from oracle import nerf_oracle as O
    return O.pose_spherical(20.0, -30.0, 4.0)[:3].contiguous().cuda()


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert (torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]), k


@pytest.mark.parametrize("hw", [(16, 16), (20, 28)])
@pytest.mark.parametrize("ref", [False, True], ids=["mip", "ref"])
def test_render_image_with_the_reference_camera_is_the_plain_call(hw, ref):
    from nerf_amd.camera import Camera
    from nerf_amd.procedures import render_image
    prop, net = _render_nets(ref)
    focal = (21.0, 19.5)
    kw = dict(white_bkg=True, render_depth=True, seed=77, depth_quantiles=(0.25, 0.5), render_opacity=True, render_normal=ref)
    with torch.no_grad():
        for extra in (dict(), dict(skip_empty=0.05)):
            plain = render_image(net, prop, _pose(), hw, focal, NEAR, FAR, 64, **kw, **extra)
            cam = render_image(net, prop, _pose(), hw, 12345.0, NEAR, FAR, 64, **kw, **extra, camera=Camera.reference(hw[0], hw[1], focal))
            assert {"rgb", "depth_img", "depth_quantiles", "opacity_img"} <= set(plain) and ("normal_img" in plain) == ref
            assert ("alive_img" in plain) == bool(extra)
            _same(plain, cam)


@pytest.mark.parametrize("hw", [(16, 16), (20, 28), (35, 30)])
def test_render_image_with_a_distorted_camera_is_render_rays_on_the_new_table(hw):
    """... in tile order: 35 x 30 is one 30 x 30 tile and a remainder of five rows the image leaves black; three uneven shards reproduce
    the single call bit for bit"""
    from nerf_amd import ops
    from nerf_amd.procedures import RENDER_COARSE_PNUM, get_patch_size, render_image
    Hh, Ww = hw
    prop, mip = _render_nets()
    row = R.cameras(Hh, Ww)["opencv"]
    R.admit(row, Hh, Ww)
    cam = R.camera_of(row)
    pose = _pose()
    kw = dict(white_bkg=True, render_depth=True, seed=77, depth_quantiles=(0.5,), render_opacity=True, camera=cam)
    with torch.no_grad():
        img = render_image(mip, prop, pose, hw, 1.0, NEAR, FAR, 64, **kw)
        rays = ops.generate_camera_rays(pose, Hh, Ww, cam, pose.device)
        sz, patch = get_patch_size(hw)
        if sz is not None:
            pr, pc = patch
            rays = rays.view(Hh, Ww, 6)[: pr * sz].reshape(pr, sz, pc, sz, 6).permute(0, 2, 1, 3, 4).reshape(-1, 6).contiguous()
        n = rays.shape[0]
        prec = ops.current_precision()
        z_base = torch.linspace(NEAR, FAR, RENDER_COARSE_PNUM).cuda()
        out = ops.render_rays(prop.packed(prec), mip.packed(prec), prec, rays, z_base, None, None, 64, NEAR, FAR, True, want_depth=True, seed=77)
        rgb, depth = out[:2]
        if sz is None:
            assert torch.equal(img["rgb"], rgb.view(Hh, Ww, 3).permute(2, 0, 1)) and torch.equal(img["depth_img"][0], depth.view(Hh, Ww))
        else:
            assert (sz, patch, n) == (30, (1, 1), 900)
            assert torch.equal(img["rgb"][:, :30], rgb.view(30, 30, 3).permute(2, 0, 1)) and not img["rgb"][:, 30:].any()
            assert torch.equal(img["depth_img"][0, :30], depth.view(30, 30))
        other = render_image(mip, prop, pose, hw, 1.0, NEAR, FAR, 64, **dict(kw, camera=R.camera_of(R.cameras(Hh, Ww)["pinhole"])))
        assert not torch.equal(other["rgb"], img["rgb"])
        cuts = (0, n // 5 + 3, n // 2 + 7, n)
        parts = [render_image(mip, prop, pose, hw, 1.0, NEAR, FAR, 64, _shard=(a, b), **kw) for a, b in zip(cuts, cuts[1:])]
    to_image = parts[0]["to_image"]
    assert torch.equal(to_image(torch.cat([p["rgb_rays"] for p in parts]), 3), img["rgb"])
    assert torch.equal(to_image(torch.cat([p["depth_rays"] for p in parts]).unsqueeze(-1), 1)[0], img["depth_img"][0])
    assert torch.equal(to_image(torch.cat([p["depth_q_rays"] for p in parts]), 1), img["depth_quantiles"])
    assert torch.equal(to_image(torch.cat([p["opacity_rays"] for p in parts]).unsqueeze(-1), 1)[0], img["opacity_img"])


def test_render_image_ipe_radius_comes_from_the_camera():
    from nerf_amd.procedures import render_image
    prop, mip = _render_nets()
    cam = R.camera_of(R.cameras(16, 16)["opencv"])
    kw = dict(white_bkg=True, seed=77, camera=cam)
    with torch.no_grad():
        a = render_image(mip, prop, _pose(), 16, 999.0, NEAR, FAR, 64, ipe=True, **kw)
        b = render_image(mip, prop, _pose(), 16, 999.0, NEAR, FAR, 64, ipe=2.0 / (12.0 ** 0.5) / cam.fx, **kw)
        c = render_image(mip, prop, _pose(), 16, 999.0, NEAR, FAR, 64, ipe=2.0 / (12.0 ** 0.5) / 999.0, **kw)
    assert torch.equal(a["rgb"], b["rgb"]) and not torch.equal(a["rgb"], c["rgb"])


# ------------------------------------------------------------------------------------------------ 4. TrainStep
def _scene8(V=3, side=8):
    from oracle import nerf_oracle as O
    gen = torch.Generator().manual_seed(17)
    images = torch.rand(V, 3, side, side, generator=gen).cuda()
    poses = torch.stack([O.pose_spherical(20.0 + 40.0 * v, -30.0, 4.0)[:3] for v in range(V)]).contiguous().cuda()
    return images, poses


def _train_step(lr=1e-3, **kw):
    from nerf_amd.optim import Adam
    from nerf_amd.training import TrainStep
    prop, mip = _nets()
    opt = Adam(list(mip.parameters()) + list(prop.parameters()), lr=lr, lr_on_device=True)
    args = dict(ray_num=96, coarse_pnum=32, fine_pnum=64, seed=1234, scene=_scene8())
    args.update(kw)
    return TrainStep(prop, mip, opt, (8, 8), (FY, FX), NEAR, FAR, **args), list(mip.parameters()) + list(prop.parameters())


def test_train_step_with_the_sampler_reference_cameras_is_the_plain_step():
    from nerf_amd.camera import Camera
    cam = Camera.reference(8, 8, (FY, FX), sampler=True)
    res = []
    for cameras in (None, cam, [cam] * 3):
        st, params = _train_step(cameras=cameras)
        assert (st.cameras is None) == (cameras is None)
        losses = []
        for _ in range(3):
            loss, img_loss = st()
            losses.append((loss.clone(), img_loss.clone(), st.ray_index.clone()))
        torch.cuda.synchronize()
        assert torch.isfinite(st.loss).item()
        res.append((losses, [p.detach().clone() for p in params]))
    for losses, params in res[1:]:
        assert all(torch.equal(x, y) for a, b in zip(losses, res[0][0]) for x, y in zip(a, b))
        assert all(torch.equal(a, b) for a, b in zip(params, res[0][1]))


def test_train_step_draws_its_rays_through_each_views_camera(monkeypatch):
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    rows = _scene_cameras(8, 8)
    st, _ = _train_step(cameras=[R.camera_of(r) for r in rows])
    assert torch.equal(st.cameras, Camera.table([R.camera_of(r) for r in rows], st.cameras.device))
    seen = []
    real = ops.sample_scene_rays

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw.get("cameras"), out[3].clone()))
        return out

    monkeypatch.setattr(ops, "sample_scene_rays", spy)
    st()
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][0] is st.cameras
    rays = seen[0][1]
    v, row, col = _decode(st.ray_index, 8, 8)
    assert torch.unique(v).numel() == 3
    _, poses = _scene8()
    for vi in range(3):
        m = v == vi
        _check_rays("view %d" % vi, rows[vi], poses[vi].cpu().numpy(), col[m].cpu().numpy(), row[m].cpu().numpy(), rays[m], "TrainStep")
    # a (V, 12) device table is taken as it is
    table = st.cameras.clone()
    st2, _ = _train_step(cameras=table)
    assert st2.cameras is table


def test_train_step_with_cameras_replayed_equals_eager():
    """capture() (one eager warm-up step) then two replays against three eager steps from the same seed: the draws are exact functions of
    the seed and the table (bit-equal indices); the parameters by the criterion the project's other replay tests apply to the same step
    without cameras (test_train_step_scene_replayed_equals_eager: 2e-5 of the parameter scale at lr 1e-5)"""
    rows = _scene_cameras(8, 8)
    res = []
    for graphed in (False, True):
        st, params = _train_step(lr=1e-5, cameras=[R.camera_of(r) for r in rows])
        drawn = []
        if graphed:
            st.capture(warmup=1)
            drawn.append(None)                                      # (the warm-up step's draw is overwritten by the recording pass's buffers)
        else:
            st()
            drawn.append(None)
        for _ in range(2):
            st()
            drawn.append(st.ray_index.clone())
        torch.cuda.synchronize()
        assert torch.isfinite(st.loss).item()
        res.append((drawn, [p.detach().clone() for p in params], st.loss.item()))
    (de, pe, le), (dg, pg, lg) = res
    assert all(torch.equal(a, b) for a, b in zip(de[1:], dg[1:])) and not torch.equal(dg[1], dg[2])
    worst = max((a - b).abs().max().item() / max(1.0, b.abs().max().item()) for a, b in zip(pg, pe))
    print("TrainStep(cameras=...) replayed vs eager: worst parameter difference / scale %.3e, loss %.9g vs %.9g" % (worst, lg, le))
    assert worst <= 2e-5 and abs(lg - le) <= 1e-5 * max(1.0, abs(le))


def test_train_step_cameras_without_a_scene_raise():
    from nerf_amd.camera import Camera
    with pytest.raises(ValueError, match="one-view scene"):
        _train_step(scene=None, cameras=Camera.reference(8, 8, FX, sampler=True))
    with pytest.raises(ValueError, match="one Camera per view"):
        _train_step(cameras=[Camera.reference(8, 8, FX, sampler=True)] * 2)
