"""Camera model, host side (no GPU): the convergence condition on the test cameras, the checks of camera_ref.py against planted faults,
nerf_amd.camera.Camera, and the argument validation of the two C entry points (before any HIP call)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import camera_ref as R

H, W = 33, 47
ONE = 0x1000                                    # any non-NULL address: a call that is rejected never dereferences it
POSE_I = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.5], [0, 0, 1, 2.0]], dtype=np.float32)          # d = (xu, -yu, -1) exactly


def pose_general():
    c, s = np.cos(0.7), np.sin(0.7)
    return np.array([[c, -s * 0.6, s * 0.8, 1.5], [s, c * 0.6, -c * 0.8, -2.0], [0.0, 0.8, 0.6, 3.0]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ the convergence condition
@pytest.mark.parametrize("name", ["opencv", "simple_radial"])
def test_convergence_condition_on_the_test_cameras(name):
    """over every pixel up to the image corner: det J > 0.3, the fp64 residual after the fixed steps < 1e-12, the radius as stated, and
    the precondition of the bound (the last fp32 correction is below DELTA_LAST)"""
    row = R.cameras()[name]
    R.admit(row, H, W)
    R.admit(R.cameras(9, 11)[name], 9, 11)                                 # (the scene-sampler test's size)
    if name == "opencv":
        assert row[4:9].astype(np.float32).tolist() == np.array([-0.12, 0.03, -0.004, 0.002, -0.0015], dtype=np.float32).tolist()


def test_constants_are_the_headers():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_amd.h")).read()
    assert "#define NERF_AMD_CAMERA_NEWTON_STEPS %d\n" % R.NEWTON_STEPS in src
    assert "#define NERF_AMD_CAMERA_DET_EPS 1e-6f\n" in src and R.DET_EPS == 1e-6
    assert "#define NERF_AMD_CAMERA_ROW 12\n" in src


# ------------------------------------------------------------------------------------------------ the checks against planted faults
def _ratios(row, **fault):
    cols, rows = R.grid(H, W)
    k = R.kernel_model(POSE_I, row, cols, rows, **fault)
    g = R.kernel_model(pose_general(), row, cols, rows, **fault)
    return R.backward_ratio(row, cols, rows, k[:, 3], -k[:, 4]), R.direction_ratio(pose_general(), row, cols, rows, g[:, 3:])


@pytest.mark.parametrize("name", ["opencv", "simple_radial"])
def test_the_restated_kernel_passes_both_checks(name):
    b, d = _ratios(R.cameras()[name])
    print("camera %s: host restatement backward err/tol %.3f, direction err/tol %.3f" % (name, b, d))
    assert b <= 1.0 and d <= 1.0


@pytest.mark.parametrize("fault", [dict(swap_p=True), dict(half=False), dict(flip=False), dict(drop_k3=True), dict(steps=R.NEWTON_STEPS - 1),
                                   dict(cx=W / 2.0)], ids=lambda f: next(iter(f)))
def test_planted_faults_are_caught(fault):
    """on the strong-distortion camera each fault fails the backward check AND the direction check"""
    b, d = _ratios(R.cameras()["opencv"], **fault)
    print("fault %s: backward err/tol %.3g, direction err/tol %.3g" % (fault, b, d))
    assert b > 1.0 and d > 1.0


def test_pinhole_restatement():
    """no coefficient: no iteration, the point is the fp32 pixel point itself and the direction check passes; the row-independent
    principal point W/2 is caught"""
    row = R.cameras()["pinhole"]
    cols, rows = R.grid(H, W)
    k = R.kernel_model(POSE_I, row, cols, rows)
    xdh, ydh = R.pixel_plane32(row, cols, rows)
    assert np.array_equal(k[:, 3].astype(np.float64), xdh) and np.array_equal(-k[:, 4].astype(np.float64), ydh)
    g = R.kernel_model(pose_general(), row, cols, rows)
    assert R.direction_ratio(pose_general(), row, cols, rows, g[:, 3:]) <= 1.0
    g = R.kernel_model(pose_general(), row, cols, rows, cx=W / 2.0)
    assert R.direction_ratio(pose_general(), row, cols, rows, g[:, 3:]) > 1.0


def test_reference_cameras_restate_todays_rays():
    """Camera.reference: the numerators of both of today's tables, exactly (small integers and halves)"""
    from nerf_amd.camera import Camera
    for Hh, Ww in ((5, 7), (8, 6)):
        cols, rows = R.grid(Hh, Ww)
        a = R.row32(Camera.reference(Hh, Ww, 10.0))
        assert np.array_equal(cols + 0.5 - a[2], (cols - Ww * 0.5) + 0.5) and np.array_equal(-(rows + 0.5 - a[3]), (Hh * 0.5 - rows) + 0.5)
        s = R.row32(Camera.reference(Hh, Ww, (11.0, 10.0), sampler=True))
        assert np.array_equal(cols + 0.5 - s[2], (cols - Ww // 2) + 0.5) and np.array_equal(-(rows + 0.5 - s[3]), (Hh // 2 - rows) + 0.5)
        assert (s[0], s[1]) == (10.0, 11.0) and not s[4:].any()


# ------------------------------------------------------------------------------------------------ nerf_amd.camera.Camera
def test_from_colmap_parameter_order_and_rejections():
    from nerf_amd.camera import Camera
    assert Camera.from_colmap("SIMPLE_PINHOLE", [500, 320, 240]).row() == [500, 500, 320, 240, 0, 0, 0, 0, 0, 0, 0, 0]
    assert Camera.from_colmap("PINHOLE", [500, 510, 320, 240]).row() == [500, 510, 320, 240, 0, 0, 0, 0, 0, 0, 0, 0]
    assert Camera.from_colmap("SIMPLE_RADIAL", [500, 320, 240, -0.1]).row() == [500, 500, 320, 240, -0.1, 0, 0, 0, 0, 0, 0, 0]
    assert Camera.from_colmap("RADIAL", [500, 320, 240, -0.1, 0.02]).row() == [500, 500, 320, 240, -0.1, 0.02, 0, 0, 0, 0, 0, 0]
    assert Camera.from_colmap("OPENCV", [500, 510, 320, 240, -0.1, 0.02, 0.003, -0.004]).row() == [500, 510, 320, 240, -0.1, 0.02, 0, 0.003, -0.004, 0, 0, 0]
    assert Camera.from_colmap("opencv", [500, 510, 320, 240, 0, 0, 0, 0]).row()[:4] == [500, 510, 320, 240]
    for model in ("FULL_OPENCV", "OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE", "FOV"):
        with pytest.raises(ValueError, match=model):
            Camera.from_colmap(model, [1.0] * 12)
    with pytest.raises(ValueError, match="4 parameters"):
        Camera.from_colmap("PINHOLE", [500, 320, 240])
    for bad in (dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")), dict(k1=float("inf"))):
        kw = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            Camera(**kw)


def test_scaled_table_row_and_distort():
    from nerf_amd.camera import ROW, Camera
    cam = Camera(500, 510, 320.5, 240.25, -0.1, 0.02, -0.003, 0.004, -0.005)
    half = cam.scaled(0.5)
    assert half.row() == [250, 255, 160.25, 120.125, -0.1, 0.02, -0.003, 0.004, -0.005, 0, 0, 0] and ROW == 12 and len(cam.row()) == 12
    with pytest.raises(ValueError):
        cam.scaled(0.0)
    t = Camera.table([cam, half], "cpu")
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 12)
    assert torch.equal(t, torch.tensor([cam.row(), half.row()], dtype=torch.float32))
    with pytest.raises(ValueError):
        Camera.table([], "cpu")
    with pytest.raises(ValueError):
        Camera.table([cam, 3.0], "cpu")
    # a resized image sees the same scene: pixel p of the half image is the ray of pixel-coordinate 2 p of the full one
    row, rh = np.asarray(cam.row()), np.asarray(half.row())
    xd, yd = R.pixel_plane(rh, np.array([10.0]), np.array([20.0]))
    xf = ((2 * 10.5 - row[2]) / row[0], (2 * 20.5 - row[3]) / row[1])
    assert abs(xd[0] - xf[0]) < 1e-15 and abs(yd[0] - xf[1]) < 1e-15
    # distort is the forward model of the specification
    x, y = torch.linspace(-0.6, 0.6, 7, dtype=torch.float64), torch.linspace(0.5, -0.4, 7, dtype=torch.float64)
    xd, yd = cam.distort(x, y)
    wx, wy = R.distort(row, x.numpy(), y.numpy())
    assert np.abs(xd.numpy() - wx).max() < 1e-15 and np.abs(yd.numpy() - wy).max() < 1e-15
    assert cam.distort(0.0, 0.0) == (0.0, 0.0)


def test_python_surface():
    from nerf_amd import ops, parallel, procedures
    from nerf_amd.training import TrainStep
    p = inspect.signature(ops.generate_camera_rays).parameters
    assert list(p) == ["pose", "H", "W", "camera", "device", "ray_offset", "n"] and p["ray_offset"].default == 0 and p["n"].default is None
    p = inspect.signature(ops.sample_scene_rays).parameters
    assert list(p)[-1] == "cameras" and p["cameras"].default is None
    for fn in (procedures.render_image, parallel.render_image_sharded):
        p = inspect.signature(fn).parameters
        # (keyword-only, so its place carries no meaning: it sits with skip_empty, ahead of the two names an older signature test reads last)
        assert p["camera"].default is None and p["camera"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(TrainStep.__init__).parameters
    assert p["cameras"].default is None and p["cameras"].kind is inspect.Parameter.KEYWORD_ONLY        # (next to scene and view_ids)


# ------------------------------------------------------------------------------------------------ the C entry points' validation
def _row(**kw):
    vals = dict(fx=10.0, fy=11.0, cx=3.5, cy=2.5, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0, r0=0.0, r1=0.0, r2=0.0)
    vals.update(kw)
    return (C.c_float * 12)(*vals.values())


def _generate(lib, pose=True, row=None, H=5, W=7, off=0, N=35, rays=ONE):
    pose = (C.c_float * 12)(*[0.0] * 12) if pose else None
    rc = lib.nerf_amd_generate_rays_camera(pose, H, W, row, off, N, rays, None)
    return rc, lib.nerf_amd_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(pose=False), "pose_host"), (dict(rays=None), "rays"), (dict(row=None), "camera is NULL"), (dict(H=0), "H, W"), (dict(W=-1), "H, W"),
    (dict(off=-1), "ray range"), (dict(N=-1), "ray range"), (dict(off=30, N=6), "ray range"),
    (dict(row=_row(fx=0.0)), "fx, fy"), (dict(row=_row(fy=-2.0)), "fx, fy"), (dict(row=_row(fx=float("nan"))), "non-finite"),
    (dict(row=_row(cy=float("inf"))), "non-finite"), (dict(row=_row(p2=float("-inf"))), "non-finite"),
    (dict(row=_row(r0=1.0)), "reserved"), (dict(row=_row(r2=-1e-30)), "reserved"),
])
def test_generate_rays_camera_rejects_bad_arguments_before_any_hip_call(kw, word):
    from nerf_amd import _lib
    kw = dict(kw)
    kw.setdefault("row", _row())
    rc, msg = _generate(_lib.lib, **kw)
    assert rc == -1, (kw, rc)
    assert msg.startswith("nerf_amd_generate_rays_camera:") and word in msg, (kw, msg)


def test_zero_rays_return_ok_without_a_launch():
    from nerf_amd import _lib
    assert _generate(_lib.lib, row=_row(), N=0)[0] == 0
    assert _lib.lib.nerf_amd_version() == 125                 # additive: the ABI number stays


def _scene(lib, **kw):
    a = dict(images=ONE, poses=ONE, V=3, H=5, W=7, view_ids=None, K=3, x0=0, x1=7, y0=0, y1=5, cameras=ONE, near=2.0, far=6.0, N=8, C=4,
             seed=1, seed_dev=None, pts=ONE, lengths=ONE, rgb=ONE, rays=ONE, index=None, stream=None)
    a.update(kw)
    rc = lib.nerf_amd_sample_scene_rays_camera(a["images"], a["poses"], a["V"], a["H"], a["W"], a["view_ids"], a["K"], a["x0"], a["x1"], a["y0"], a["y1"],
                                               a["cameras"], a["near"], a["far"], a["N"], a["C"], a["seed"], a["seed_dev"], a["pts"], a["lengths"],
                                               a["rgb"], a["rays"], a["index"], a["stream"])
    return rc, lib.nerf_amd_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(images=None), "images"), (dict(poses=None), "poses"), (dict(cameras=None), "cameras"), (dict(rgb=None), "rgb"), (dict(rays=None), "rays"),
    (dict(K=0), "K"), (dict(K=4), "K"), (dict(V=0), "V"), (dict(x0=3, x1=3), "x0"), (dict(x1=8), "x1"), (dict(y0=2, y1=2), "y0"), (dict(y1=6), "y1"),
    (dict(N=-1), "N"), (dict(C=-1), "C"), (dict(lengths=None), "pts"), (dict(pts=None), "lengths"),
])
def test_sample_scene_rays_camera_rejects_bad_arguments_before_any_hip_call(kw, word):
    from nerf_amd import _lib
    rc, msg = _scene(_lib.lib, **kw)
    assert rc == -1, (kw, rc)
    assert msg.startswith("nerf_amd_sample_scene_rays_camera") and word in msg.split(":", 1)[1], (kw, msg)
    assert _scene(_lib.lib, N=0)[0] == 0


def test_train_step_cameras_need_a_scene_and_cpu_forms_are_rejected():
    from nerf_amd import ops
    from nerf_amd.camera import Camera
    cam = Camera(10, 10, 3.5, 2.5)
    with pytest.raises(ValueError, match="one Camera per view"):
        ops.scene_cameras([cam, cam], 3, "cpu")
    with pytest.raises(ValueError, match="cameras"):
        ops.scene_cameras(torch.zeros(3, 12), 3, "cpu")                  # a table must already be on the device
    assert ops.scene_cameras(None, 3, "cpu") is None
    assert torch.equal(ops.scene_cameras(cam, 3, "cpu"), Camera.table([cam] * 3, "cpu"))
