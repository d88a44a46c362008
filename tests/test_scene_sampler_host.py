"""Scene sampler, host side (no GPU, no launch): nerf_amd_sample_scene_rays validates its arguments before any HIP call and names the
offending one, training.rank_seed gives the ranks of a data-parallel scene-mode run distinct seeds, and the Python surface exists with
the documented signatures."""
import inspect

import pytest
import torch

ONE = 0x1000                                    # any non-NULL address: a call that is rejected never dereferences it


def _call(lib, **kw):
    a = dict(images=ONE, poses=ONE, V=3, H=5, W=7, view_ids=None, K=3, x0=0, x1=7, y0=0, y1=5, fx=10.0, fy=10.0, near=2.0, far=6.0, N=8, C=4,
             seed=1, seed_dev=None, pts=ONE, lengths=ONE, rgb=ONE, rays=ONE, index=None, stream=None)
    a.update(kw)
    rc = lib.nerf_amd_sample_scene_rays(a["images"], a["poses"], a["V"], a["H"], a["W"], a["view_ids"], a["K"], a["x0"], a["x1"], a["y0"], a["y1"],
                                        a["fx"], a["fy"], a["near"], a["far"], a["N"], a["C"], a["seed"], a["seed_dev"], a["pts"], a["lengths"],
                                        a["rgb"], a["rays"], a["index"], a["stream"])
    return rc, lib.nerf_amd_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(images=None), "images"), (dict(poses=None), "poses"), (dict(rgb=None), "rgb"), (dict(rays=None), "rays"),
    (dict(K=0), "K"), (dict(K=4), "K"), (dict(V=0), "V"),
    (dict(x0=3, x1=3), "x0"), (dict(x0=-1), "x0"), (dict(x1=8), "x1"), (dict(x0=5, x1=2), "x0"),
    (dict(y0=2, y1=2), "y0"), (dict(y0=-1), "y0"), (dict(y1=6), "y1"),
    (dict(N=-1), "N"), (dict(C=-1), "C"), (dict(lengths=None), "pts"), (dict(pts=None), "lengths"),
])
def test_entry_point_rejects_bad_arguments_before_any_hip_call(kw, word):
    from nerf_amd import _lib
    rc, msg = _call(_lib.lib, **kw)
    assert rc == -1, (kw, rc)
    assert msg.startswith("nerf_amd_sample_scene_rays") and word in msg.split(":", 1)[1], (kw, msg)


def test_zero_rays_return_ok_without_a_launch():
    """N == 0 with otherwise valid arguments: OK, and no HIP call (there is no device here to make one on)."""
    from nerf_amd import _lib
    rc, _ = _call(_lib.lib, N=0)
    assert rc == 0
    rc, _ = _call(_lib.lib, N=0, C=0, pts=None, lengths=None)
    assert rc == 0
    assert _lib.lib.nerf_amd_version() == 125                 # additive: the ABI number stays


def test_rank_seed():
    from nerf_amd.training import rank_seed
    for seed in (0, 1, 1234, 2 ** 61 + 12345, 2 ** 62 - 1):
        assert rank_seed(seed, 0) == seed
        got = [rank_seed(seed, r) for r in range(64)]
        assert len(set(got)) == 64, seed
        assert all(0 <= g < 2 ** 62 for g in got), seed
        assert got == [rank_seed(seed, r) for r in range(64)]                # pure
    assert len({rank_seed(s, 1) for s in range(100)}) == 100                  # and the seed still matters on the other ranks
    with pytest.raises(ValueError):
        rank_seed(1, -1)


def test_python_surface():
    from nerf_amd import ops, utils
    from nerf_amd.training import TrainStep
    p = inspect.signature(ops.sample_scene_rays).parameters
    assert list(p)[:14] == ["images", "poses", "fx", "fy", "near", "far", "n_rays", "n_points", "seed", "seed_dev", "window", "view_ids", "want_samples",
                            "want_index"]
    assert p["seed"].default == 0 and p["seed_dev"].default is None and p["window"].default is None and p["view_ids"].default is None
    assert p["want_samples"].default is True and p["want_index"].default is True
    q = inspect.signature(utils.sceneSampler).parameters
    assert list(q) == ["images", "poses", "ray_num", "point_num", "focal", "near", "far", "crop_xy", "view_ids", "output_samples"]
    assert q["crop_xy"].default == (1., 1.) and q["view_ids"].default is None and q["output_samples"].default is True
    t = inspect.signature(TrainStep.__init__).parameters
    assert t["scene"].default is None and t["view_ids"].default is None


def test_crop_window_is_the_rule_of_random_from_one_image():
    """crop -> window: the bounds randomFromOneImage cuts its table with (the issue's example: 6 x 10 at (0.5, 0.5) = cols 2..6, rows 1..3)"""
    from nerf_amd.utils import crop_window, randomFromOneImage
    assert crop_window(6, 10, (0.5, 0.5)) == (2, 7, 1, 4)
    assert crop_window(5, 7, (1.0, 1.0)) == (0, 7, 0, 5)
    for H, W, crop in ((5, 7, (0.5, 0.5)), (6, 10, (0.5, 0.5)), (9, 8, (0.3, 1.0)), (5, 7, (1.0, 1.0))):
        x0, x1, y0, y1 = crop_window(H, W, crop)
        img = torch.arange(3 * H * W, dtype=torch.float32).reshape(3, H, W)
        pix, coords = randomFromOneImage(img, crop)
        rows, cols = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
        assert torch.equal(coords, torch.stack((cols - W // 2, H // 2 - rows), -1).reshape(-1, 2))
        assert torch.equal(pix, img[:, y0:y1, x0:x1].reshape(3, -1).t())


def test_cpu_tensors_and_bad_forms_are_rejected():
    from nerf_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.sample_scene_rays(torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 4), 1.0, 1.0, 2.0, 6.0, 4, 4)
    with pytest.raises(ValueError):
        ops.scene_view_ids([0, 3], 3, "cpu")
    with pytest.raises(ValueError):
        ops.scene_view_ids([-1], 3, "cpu")
    with pytest.raises(ValueError):
        ops.scene_view_ids([], 3, "cpu")
    assert ops.scene_view_ids(None, 3, "cpu") is None
    assert ops.scene_view_ids([2, 0], 3, "cpu").tolist() == [2, 0]
