"""Image metrics on the GPU (nerf_amd_image_metrics, ops.image_metrics, nerf_amd.metrics): the kernel against the fp64 specification of
tests/image_metrics_ref.py, position by position, within the bounds derived there from the shipped algorithm (err / tol <= 1 through
conftest.gate, which records every figure); the closed forms; and the properties the interface promises bit for bit -- a view does not depend
on the other views of its call, nothing depends on what the outputs and the workspace held, on a second run, on the map being asked for, or
on running from a captured graph.  Then evaluate_views against render_image + image_metrics, and render_only's output with the flag off."""
import ctypes
import os

import numpy as np
import pytest
import torch

import image_metrics_ref as R
from conftest import gate

pytestmark = pytest.mark.gpu
SEED = 20241


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")
    yield
    nerf_amd.set_precision("fp32")


def _tile():
    from nerf_amd import _lib
    return _lib.IMAGE_METRICS_TILE + (_lib.IMAGE_METRICS_SEGMENT_H,)


SHAPES = R.sweep_shapes(16, 64, 128)


def test_the_sweep_is_built_on_the_kernels_tile():
    assert SHAPES == R.sweep_shapes(*_tile())


def _np(result):
    return {k: v.detach().cpu().numpy() for k, v in result.items()}


def _run(pred, target, want_map=True):
    from nerf_amd import metrics
    return metrics.image_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(target).cuda(), want_map=want_map)


def _raw(pred, target, fill, want_map=True):
    """the C entry point on buffers whose every byte was `fill` -> (mse, ssim, map) device tensors"""
    from nerf_amd import _lib
    V, C, H, W = pred.shape
    n_ws = _lib.lib.nerf_amd_image_metrics_workspace_bytes(V, C, H, W)
    assert n_ws % 16 == 0 and n_ws > 0
    new = lambda n, dtype: torch.empty((n * torch.empty((), dtype=dtype).element_size(),), dtype=torch.uint8, device="cuda").fill_(fill).view(dtype)
    mse, ssim, ws = new(V, torch.float64), new(V, torch.float64), new(n_ws // 8, torch.float64)
    smap = new(V * C * (H - 10) * (W - 10), torch.float32) if want_map else None
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.lib.nerf_amd_image_metrics(p(pred), p(target), V, C, H, W, p(mse), p(ssim), p(smap), p(ws), torch.cuda.current_stream().cuda_stream),
               "nerf_amd_image_metrics")
    return mse, ssim, (smap.view(V, C, H - 10, W - 10) if want_map else None)


@pytest.mark.parametrize("kind", R.INPUT_KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_specification(shape, kind):
    pred, target = R.make_inputs(shape, kind)
    sp = R.spec(pred, target)
    tols = R.bounds(sp)
    assert np.isfinite(tols[0]).all()
    out = _run(pred, target)
    assert out["ssim_map"].shape == sp["ssim_map"].shape and out["ssim_map"].dtype == torch.float32
    for k in ("mse", "ssim", "psnr"):
        assert out[k].shape == (shape[0],) and out[k].dtype == torch.float64 and out[k].is_cuda
    got = _np(out)
    r = R.ratios(got, sp, tols)
    tag = "image_metrics %s %s" % ("x".join(map(str, shape)), kind)
    gate(tag + ": ssim_map err / tol, worst position", r["map"], 1.0)
    gate(tag + ": ssim[v] err / tol", r["ssim"], 1.0)
    gate(tag + ": mse[v] err / tol", r["mse"], 1.0)
    # psnr = -10 log10(mse) in fp64: the relative bound of mse is an absolute one of 10 / ln 10 times it in dB (+ fp64 rounding of the log)
    gate(tag + ": psnr err / tol", float(np.max(np.abs(got["psnr"] - sp["psnr"]) / (10.0 / np.log(10.0) * (2 * R.U + R.U ** 2 + 2.0 ** -40) * 1.01 + 1e-13))), 1.0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identical_and_constant_images(shape):
    pred, _ = R.make_inputs(shape, "textured", seed=1)
    sp = R.spec(pred, pred)
    tol_map, tol_ssim, _ = R.bounds(sp)
    out = _np(_run(pred, pred))
    assert (out["mse"] == 0.0).all() and np.isposinf(out["psnr"]).all()                      # exactly
    gate("image_metrics %s identical: |1 - ssim_map| / tol" % (shape,), float(np.max(np.abs(out["ssim_map"] - 1.0) / tol_map)), 1.0)
    gate("image_metrics %s identical: |1 - ssim[v]| / tol" % (shape,), float(np.max(np.abs(out["ssim"] - 1.0) / tol_ssim)), 1.0)
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.9, 0.9)):
        pa, pb = np.full(shape, a, np.float32), np.full(shape, b, np.float32)
        sp = R.spec(pa, pb)
        tol_map, tol_ssim, tol_mse = R.bounds(sp)
        out = _np(_run(pa, pb))
        want = R.constant_ssim(float(np.float32(a)), float(np.float32(b)))
        assert np.max(np.abs(sp["ssim_map"] - want)) <= 1e-12                                # (the closed form is the specification's value)
        tag = "image_metrics %s constants %g, %g" % (shape, a, b)
        gate(tag + ": ssim_map against the closed form / tol", float(np.max(np.abs(out["ssim_map"] - want) / tol_map)), 1.0)
        gate(tag + ": ssim[v] against the closed form / tol", float(np.max(np.abs(out["ssim"] - want) / tol_ssim)), 1.0)
        d2 = (float(np.float32(a)) - float(np.float32(b))) ** 2
        gate(tag + ": mse against (a - b)^2 / tol", float(np.max(np.abs(out["mse"] - d2) / np.maximum(d2 * (2 * R.U + R.U ** 2 + 2.0 ** -40), 1e-300))), 1.0)


def test_bit_for_bit_properties():
    """per view == single-view calls | 0x00 / 0xFF pre-fill | two runs | want_map off | (C, H, W) == (1, C, H, W)"""
    from nerf_amd import ops
    for shape in ((3, 3, 40, 56), (2, 3, 13, 75), (2, 1, _tile()[0] + 11, _tile()[1] + 11), (2, 1, _tile()[2] + 27, 75)):
        pred, target = (torch.from_numpy(a).cuda() for a in R.make_inputs(shape, "textured", seed=2))
        mse, ssim, smap = ops.image_metrics(pred, target, want_map=True)
        for v in range(shape[0]):                                                            # the multi-view call == V single-view calls
            m1, s1, map1 = ops.image_metrics(pred[v:v + 1], target[v:v + 1], want_map=True)
            assert torch.equal(m1[0], mse[v]) and torch.equal(s1[0], ssim[v]) and torch.equal(map1[0], smap[v]), (shape, v)
            m3, s3, map3 = ops.image_metrics(pred[v], target[v], want_map=True)              # (C, H, W) is V = 1
            assert torch.equal(m3, m1) and torch.equal(s3, s1) and torch.equal(map3, map1)
        for fill in (0x00, 0xFF):                                                            # nothing is accumulated into or read before it is written
            m2, s2, map2 = _raw(pred, target, fill)
            assert torch.equal(m2, mse) and torch.equal(s2, ssim) and torch.equal(map2, smap), (shape, fill)
            m2, s2, _ = _raw(pred, target, fill, want_map=False)
            assert torch.equal(m2, mse) and torch.equal(s2, ssim), (shape, fill)
        again = ops.image_metrics(pred, target, want_map=True)                               # two runs
        assert all(torch.equal(a, b) for a, b in zip(again, (mse, ssim, smap)))
        m4, s4 = ops.image_metrics(pred, target)                                             # want_map=False: the same ssim and mse bits
        assert torch.equal(m4, mse) and torch.equal(s4, ssim)
        assert not torch.equal(ssim[0], ssim[1]) and not torch.equal(mse[0], mse[1])         # (the views do differ)


def test_captured_graph_replays_on_new_inputs():
    from nerf_amd import ops
    shape = (2, 3, 40, 56)
    a_pred, a_target = (torch.from_numpy(a).cuda() for a in R.make_inputs(shape, "textured", seed=3))
    b_pred, b_target = (torch.from_numpy(a).cuda() for a in R.make_inputs(shape, "wide", seed=4))
    pred, target = a_pred.clone(), a_target.clone()
    ops.image_metrics(pred, target, want_map=True)                                           # warm
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        captured = ops.image_metrics(pred, target, want_map=True)
    pred.copy_(b_pred)                                                                       # overwritten in place, then replayed
    target.copy_(b_target)
    graph.replay()
    torch.cuda.synchronize()
    eager_b = ops.image_metrics(b_pred, b_target, want_map=True)
    eager_a = ops.image_metrics(a_pred, a_target, want_map=True)
    assert all(torch.equal(c, e) for c, e in zip(captured, eager_b))
    assert not torch.equal(eager_a[1], eager_b[1])


def test_indexing_beyond_2_to_31_elements():
    """V C H W = 2^31 elements per input (8 GiB each): the last view of the big call == that view alone, bit for bit, and == the specification.
    The other views are noise from the device generator; only offsets are under test."""
    from nerf_amd import ops
    V, C, H, W = 2 ** 31 // (64 * 128), 1, 64, 128
    assert V * C * H * W >= 2 ** 31
    gen = torch.Generator(device="cuda").manual_seed(7)
    target = torch.rand((V, C, H, W), device="cuda", generator=gen)
    pred = target.clone()
    lp, lt = R.make_inputs((1, C, H, W), "textured", seed=5)
    pred[-1:].copy_(torch.from_numpy(lp))
    target[-1:].copy_(torch.from_numpy(lt))
    mse, ssim = ops.image_metrics(pred, target)
    m1, s1 = ops.image_metrics(pred[-1:], target[-1:])
    assert torch.equal(mse[-1:], m1) and torch.equal(ssim[-1:], s1)
    assert bool((mse[:-1] == 0).all()) and float((ssim[:-1] - 1.0).abs().max()) <= 1e-4       # identical views everywhere else
    sp = R.spec(lp, lt)
    r = R.ratios({"ssim_map": sp["ssim_map"], "ssim": s1.cpu().numpy(), "mse": m1.cpu().numpy()}, sp)
    gate("image_metrics last of %d views (2^31 elements): ssim[v] err / tol" % V, r["ssim"], 1.0)
    gate("image_metrics last of %d views (2^31 elements): mse[v] err / tol" % V, r["mse"], 1.0)
    del pred, target
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ evaluate_views, render_only
def _nets():
    from nerf_amd import synthetic_weights as SW
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(SW.proposal_state("small"))
    mip.load_state_dict(SW.mip_state("small"))
    return prop.cuda().eval(), mip.cuda().eval()


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_evaluate_views_is_render_image_plus_image_metrics(precision):
    import nerf_amd
    from nerf_amd import metrics, procedures
    from nerf_amd.utils import pose_spherical
    nerf_amd.set_precision(precision)
    prop, mip = _nets()
    H, W, V = 24, 20, 2
    focal = 0.5 * W / float(np.tan(0.5 * 0.6911112070083618))
    poses_host = torch.stack([pose_spherical(40.0 * k, -30.0, 4.0) for k in range(V)])        # (V, 4, 4) on the host: what a dataset holds
    poses = poses_host[:, :3].cuda()
    images = torch.from_numpy(R.make_inputs((V, 3, H, W), "textured", seed=6)[1]).cuda()
    kw = dict(sample_num=16, white_bkg=True)
    with torch.no_grad():
        stacked = torch.stack([procedures.render_image(mip, prop, poses[v], (H, W), focal, 2.0, 6.0, 16, white_bkg=True, rng="philox", seed=SEED + v)["rgb"]
                               for v in range(V)]).contiguous()
        want = metrics.image_metrics(stacked, images)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                                              # no device-to-host copy, no synchronisation
        try:
            got = metrics.evaluate_views(mip, prop, images, poses_host, focal, 2.0, 6.0, seed=SEED, rng="philox", **kw)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        on_device = metrics.evaluate_views(mip, prop, images, poses, focal, 2.0, 6.0, seed=SEED, rng="philox", **kw)   # device poses: the same bits
    assert all(torch.equal(on_device[k], got[k]) for k in got)
    assert set(got) == {"mse", "psnr", "ssim", "mean_psnr", "mean_ssim"}
    for k in ("mse", "psnr", "ssim"):
        assert got[k].is_cuda and got[k].dtype == torch.float64 and torch.equal(got[k], want[k]), k
    for k in ("psnr", "ssim"):
        assert got["mean_" + k].shape == () and got["mean_" + k].dtype == torch.float64 and got["mean_" + k].is_cuda
        assert torch.equal(got["mean_" + k], want[k].mean())
    assert bool(torch.isfinite(got["psnr"]).all()) and not torch.equal(got["ssim"][0], got["ssim"][1])
    # and the values are the specification's on the rendered images
    sp = R.spec(stacked.cpu().numpy(), images.cpu().numpy())
    r = R.ratios({"ssim_map": sp["ssim_map"], "ssim": got["ssim"].cpu().numpy(), "mse": got["mse"].cpu().numpy()}, sp)
    gate("evaluate_views %s: ssim[v] err / tol" % precision, r["ssim"], 1.0)
    gate("evaluate_views %s: mse[v] err / tol" % precision, r["mse"], 1.0)


def test_render_only_output_with_the_flag_off_and_on(tmp_path, capsys, monkeypatch):
    """flag off: stdout is exactly the per-view lines of before -- rebuilt here with SoftL1Loss and LossPSNR from the images the run rendered --
    and nothing else; flag on: the same lines, one SSIM line after each, one summary line at the end, the same renders and the same PNG bytes."""
    import json
    from PIL import Image
    import nerf_amd
    from nerf_amd import metrics, procedures
    from nerf_amd.addtional import LossPSNR, SoftL1Loss
    from nerf_amd.dataset import AdaptiveResize, CustomDataSet, to_tensor
    from nerf_amd.nerf_helper import saveModel
    from nerf_amd.utils import pose_spherical
    nerf_amd.set_precision(None)
    root = str(tmp_path)
    scene = os.path.join(root, "data", "toy")
    os.makedirs(os.path.join(scene, "test"))
    frames = []
    for k in range(2):
        gt = (R.make_inputs((50, 50, 3), "textured", seed=8 + k)[1] * 255).astype(np.uint8)
        Image.fromarray(gt).save(os.path.join(scene, "test", "r_%d.png" % k))
        frames.append({"file_path": "./test/r_%d" % k, "transform_matrix": pose_spherical(40.0 * k, -30.0, 4.0).tolist()})
    json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(os.path.join(scene, "transforms_test.json"), "w"))
    prop, mip = _nets()
    os.makedirs(os.path.join(root, "model"))
    saveModel(mip, os.path.join(root, "model", "toy_mip.pth"))
    saveModel(prop, os.path.join(root, "model", "toy_prop.pth"))
    rendered = []
    real_render = procedures.render_image

    def spy(*args, **kw):                                                                    # calls through; keeps the image each view rendered
        out = real_render(*args, **kw)
        rendered.append(out["rgb"].clone())
        return out

    monkeypatch.setattr(procedures, "render_image", spy)
    base = ["--name", "toy", "--dataset_name", "toy", "--img_scale", "1.0", "--opt_mode", "none", "-e", "-w"]
    texts, pngs, images = {}, {}, {}
    for flag in (False, True):
        out_root = os.path.join(root, "out_%d" % flag) + "/"
        torch.manual_seed(3)
        del rendered[:]
        procedures.render_only(procedures.get_parser().parse_args(base + (["--eval_ssim"] if flag else [])), os.path.join(root, "model") + "/", "O1",
                               dataset_root=os.path.join(root, "data") + "/", output_root=out_root)
        texts[flag] = capsys.readouterr().out
        images[flag] = list(rendered)
        pngs[flag] = [open(os.path.join(out_root, "given", "result_%03d.png" % k), "rb").read() for k in range(2)]
    assert len(images[False]) == len(images[True]) == 2 and all(torch.equal(a, b) for a, b in zip(images[False], images[True]))
    resize = AdaptiveResize(1.0)
    testset = CustomDataSet(scene + "/", lambda im: to_tensor(resize(im)), 1.0, False, use_alpha=False)      # the ground truth as render_only loads it
    old_lines, ssim_lines, rows = [], [], []
    with torch.no_grad():
        for k in range(2):
            rgb, gt = images[False][k], testset[k][0].cuda()
            loss = SoftL1Loss()(rgb, gt)
            old_lines.append("Image loss:%.6f\tPSNR:%.4f" % (loss.item(), LossPSNR()(loss).item()))
            m = metrics.image_metrics(rgb.float().contiguous(), gt.float().contiguous())
            ssim_lines.append("Image SSIM:%.6f" % m["ssim"][0].item())
            rows.append((m["psnr"][0].item(), m["ssim"][0].item()))
    off, on = texts[False].splitlines(), texts[True].splitlines()
    assert len(off) == 4 and all(l.startswith("NeRF Model loaded from") for l in off[:2]) and off[:2] == on[:2]   # (the two checkpoint loaders' lines)
    assert off[2:] == old_lines and texts[False].endswith(old_lines[1] + "\n"), texts[False]   # byte for byte, and not one line more
    summary = "Test set (2 views): mean PSNR:%.4f\tmean SSIM:%.6f" % (sum(r[0] for r in rows) / 2, sum(r[1] for r in rows) / 2)
    assert on[2:] == [old_lines[0], ssim_lines[0], old_lines[1], ssim_lines[1], summary], texts[True]
    assert 0.0 < rows[0][1] < 0.5 and rows[0][1] != rows[1][1]
    assert pngs[False] == pngs[True]
