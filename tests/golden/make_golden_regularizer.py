#!/usr/bin/env python3
"""Golden G26: the REAL reference's ``nerf.addtional.Regularizer`` (addtional.py:26-35) on CPU in fp32 -- inputs, loss and
``torch.autograd.grad`` w.r.t. both inputs -- for the distortion-loss kernels (nerf_amd_distortion_loss, mode 0).  It needs a checkout of
the reference (make_golden.py's REF); the tests read only the .npz written here:

    python tests/golden/make_golden_regularizer.py

Cases (prefix of the stored arrays):
  pipe    128 rays x 128 sorted depths in [2, 6] with rendered-weight-like w (alpha compositing of a peaked density)
  unsort  37 rays x 7 depths in no order, one depth tied with another in every row (sgn(0) = 0 in the gradient of |x|)
  nan     4 rays x 2 depths: one interval, r = 0, the reference's 0/0 = NaN
  s257    8 rays x 257 sorted depths
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import install_shims, npz  # noqa: E402


def rendered_like(n, s, g):
    t = torch.sort(2.0 + 4.0 * torch.rand(n, s, generator=g), dim=-1)[0]
    peak = 2.5 + 3.0 * torch.rand(n, 1, generator=g)
    width = 0.05 + 0.4 * torch.rand(n, 1, generator=g)
    sigma = 40.0 * torch.exp(-((t - peak) / width) ** 2) + 0.05 * torch.rand(n, s, generator=g)
    delta = torch.cat((t[:, 1:] - t[:, :-1], torch.full((n, 1), 1e10)), -1)
    alpha = 1.0 - torch.exp(-sigma * delta)
    trans = torch.cumprod(torch.cat((torch.ones(n, 1), 1.0 - alpha + 1e-10), -1), -1)[:, :-1]
    return (alpha * trans).float(), t.float()


def main():
    install_shims()
    from nerf.addtional import Regularizer
    reg = Regularizer()
    g = torch.Generator().manual_seed(26)
    cases = {}
    cases["pipe"] = rendered_like(128, 128, g)
    t = 2.0 + 4.0 * torch.rand(37, 7, generator=g)
    t[:, 5] = t[:, 2]
    cases["unsort"] = (torch.rand(37, 7, generator=g), t)
    cases["nan"] = (torch.rand(4, 2, generator=g), torch.sort(2.0 + 4.0 * torch.rand(4, 2, generator=g), dim=-1)[0])
    cases["s257"] = rendered_like(8, 257, g)
    out = {}
    for name, (w, t) in cases.items():
        w = w.float().contiguous().requires_grad_(True)
        t = t.float().contiguous().requires_grad_(True)
        loss = reg(w, t)
        gw, gt = torch.autograd.grad(loss, (w, t))
        out.update({name + "_w": w.detach(), name + "_t": t.detach(), name + "_loss": loss.detach(), name + "_gw": gw, name + "_gt": gt})
        print("%-7s N=%3d S=%3d  loss %.8g" % (name, w.shape[0], w.shape[1], loss.item()))
    npz("g26_regularizer", **out)


if __name__ == "__main__":
    main()
