"""Distortion regularisers, host side (no GPU): the reference's Regularizer is mirrored (signature, shim, the CPU evaluation against golden
G26 written from the real reference), Mip-NeRF 360's DistortionLoss evaluates its definition on CPU tensors, and TrainStep takes the
`distortion` keyword."""
import inspect
import os
import subprocess
import sys

import torch

import sigtools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("pipe", "unsort", "nan", "s257")


def test_regularizer_and_distortion_loss_are_importable():
    from nerf_amd.addtional import DistortionLoss, Regularizer
    assert issubclass(Regularizer, torch.nn.Module) and issubclass(DistortionLoss, torch.nn.Module)


def test_shim_serves_the_regularizer():
    """`from nerf.addtional import Regularizer` in a fresh interpreter with only <root>:<root>/compat on the path."""
    compat = os.path.join(ROOT, "compat")
    code = ("import sys, nerf.addtional as shim, nerf_amd.addtional as real\n"
            "assert shim.__file__.startswith(sys.argv[1]), shim.__file__\n"
            "from nerf.addtional import Regularizer\n"
            "assert Regularizer is real.Regularizer and shim.DistortionLoss is real.DistortionLoss\n"
            "print('resolved')\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, compat]))
    r = subprocess.run([sys.executable, "-c", code, compat], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "resolved" in r.stdout, r.stderr[-2000:]


def test_regularizer_signatures_equal_g20(golden):
    from nerf_amd import addtional
    want = golden("g20_signatures")["addtional"]
    have = sigtools.module_signatures(addtional, "addtional")
    for key in ("Regularizer", "Regularizer.__init__", "Regularizer.forward"):
        assert have[key] == want[key], (key, have.get(key), want[key])


def test_regularizer_cpu_equals_g26(golden):
    """CPU tensors evaluate the reference's expression: loss and autograd gradients equal G26 (the reference in fp32)."""
    from nerf_amd.addtional import Regularizer
    g = golden("g26_regularizer")
    for c in CASES:
        w = g[c + "_w"].clone().requires_grad_(True)
        t = g[c + "_t"].clone().requires_grad_(True)
        loss = Regularizer()(w, t)
        gw, gt = torch.autograd.grad(loss, (w, t))
        want = torch.tensor(g[c + "_loss"])
        if c == "nan":
            assert torch.isnan(loss).item() and torch.isnan(want).item()
            assert torch.equal(torch.isnan(gw), torch.isnan(g[c + "_gw"])) and torch.equal(torch.isnan(gt), torch.isnan(g[c + "_gt"]))
            continue
        assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()), c
        assert torch.allclose(gw, g[c + "_gw"], rtol=1e-5, atol=1e-6 * g[c + "_gw"].abs().max().item()), c
        assert torch.allclose(gt, g[c + "_gt"], rtol=1e-5, atol=1e-6 * g[c + "_gt"].abs().max().item()), c


def test_distortion_loss_cpu_is_the_definition():
    """DistortionLoss on CPU tensors = (1/N) sum_rays [sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 d_i / 3], written out as loops here."""
    from nerf_amd.addtional import DistortionLoss
    gen = torch.Generator().manual_seed(0)
    e = torch.sort(torch.rand(5, 9, generator=gen, dtype=torch.float64), dim=-1)[0]
    w = torch.rand(5, 8, generator=gen, dtype=torch.float64)
    total = 0.0
    for n in range(5):
        m = [(e[n, i] + e[n, i + 1]).item() / 2 for i in range(8)]
        total += sum(w[n, i].item() * w[n, j].item() * abs(m[i] - m[j]) for i in range(8) for j in range(8))
        total += sum(w[n, i].item() ** 2 * (e[n, i + 1] - e[n, i]).item() for i in range(8)) / 3
    assert abs(DistortionLoss()(w, e).item() - total / 5) <= 1e-12
    assert abs(DistortionLoss(0.25)(w, e).item() - 0.25 * total / 5) <= 1e-12


def test_train_step_signature_ends_in_distortion():
    from nerf_amd.training import TrainStep
    params = list(inspect.signature(TrainStep.__init__).parameters.values())
    assert params[-1].name == "distortion" and params[-1].default == 0.0
    assert params[-2].name == "grad_clip"


def test_distortion_abi_validates_before_any_hip_call():
    from nerf_amd import _lib
    lib = _lib.lib
    for n, s, mode in ((4, 1, 1), (4, 1025, 1), (4, 8, 2), (-1, 8, 0)):
        assert lib.nerf_amd_distortion_loss(None, None, n, s, mode, 1.0, None, None, None) == -1
        assert lib.nerf_amd_last_error()
        assert lib.nerf_amd_distortion_loss_backward(None, None, n, s, mode, 1.0, None, None, None, None) == -1
    assert lib.nerf_amd_distortion_loss(None, None, 4, 1025, 0, 1.0, None, None, None) == -1
    assert b"1024" in lib.nerf_amd_last_error()
