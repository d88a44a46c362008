#!/usr/bin/env python3
"""Golden G27: the outputs of the two fused bf16 render kernels -- proposal density and fine (r, g, b, sigma) -- AS THE PARENT OF THE
RESIDENT-WEIGHTS CHANGE COMPUTED THEM, bit for bit.  Keeping part of the weight stream resident in LDS changes where an A fragment is
read from and nothing else, so the kernels must reproduce these numbers exactly (tests/test_gpu_resident_weights.py).

Run on an MI355X with the library built from the parent commit (NERF_AMD_LIB may point at it):

    python tests/golden/make_golden_render_mlp.py [OUTPUT.npz]

Inputs are closed-form (the integer hash of nerf_amd.synthetic_weights), so only the outputs are stored: in full for M = 1, 255, 257 (the
ragged-tile guards around the 256-sample tile) and on a fixed sample of rows for M = 2 * 256 * 256 + 37, the smallest size at which a
persistent workgroup of a 256-CU part runs a third tile (the weight ring then wraps across tiles twice).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SIZES = (1, 255, 257, 2 * 256 * 256 + 37)
TAGS = ("small", "he")
N_ROWS = 4096                      # rows kept of the large size


def inputs(M: int) -> torch.Tensor:
    """(M, 1, 6) fp32: position in [-4, 4)^3, direction in [-1, 1)^3 -- a pure function of (M, row, column)"""
    from nerf_amd.synthetic_weights import _hash_uniform
    u = _hash_uniform(M, 6, 27000 + M % 1000)
    u[:, :3] *= 8.0
    u[:, 3:] *= 2.0
    return torch.from_numpy(u.astype(np.float32)).reshape(M, 1, 6)


def kept_rows(M: int) -> np.ndarray:
    """all rows of a small size; of a large one the first and the last 64 (the ragged last tile) and a hashed sample of the rest"""
    if M <= N_ROWS:
        return np.arange(M, dtype=np.int64)
    from nerf_amd.synthetic_weights import _hash_uniform
    pick = ((_hash_uniform(N_ROWS - 128, 1, 2727)[:, 0] + 0.5) * M).astype(np.int64) % M
    return np.unique(np.concatenate((np.arange(64), pick, np.arange(M - 64, M)))).astype(np.int64)


def render_mlp_outputs(pkg, prop, mip, M: int):
    """-> (density (M,), rgbo (M, 4)) of the bf16 kernels, fp32 on the host"""
    pts = inputs(M).cuda()
    pkg.set_precision("bf16")
    try:
        with torch.no_grad():
            d = prop.forward(pts[..., :3].contiguous())
            o = mip.forward(pts)
        torch.cuda.synchronize()
    finally:
        pkg.set_precision("fp32")
    return d.reshape(M).float().cpu(), o.reshape(M, 4).float().cpu()


def build_nets(tag: str):
    from nerf_amd import addtional, mip_model, synthetic_weights as W
    prop = addtional.ProposalNetwork(10, 256)
    mip = mip_model.MipNeRF(10, 4, 256)
    prop.load_state_dict(W.proposal_state(tag))
    mip.load_state_dict(W.mip_state(tag))
    return prop.cuda().eval(), mip.cuda().eval()


def main():
    sys.path.insert(0, ROOT)
    import nerf_amd
    out = {}
    for tag in TAGS:
        prop, mip = build_nets(tag)
        for M in SIZES:
            d, o = render_mlp_outputs(nerf_amd, prop, mip, M)
            rows = kept_rows(M)
            out["rows_%d" % M] = rows
            out["%s_%d_density" % (tag, M)] = d.numpy()[rows].view(np.int32)
            out["%s_%d_rgbo" % (tag, M)] = o.numpy()[rows].view(np.int32)
            print("%-5s M=%6d rows kept %4d  density %.6g .. %.6g  sigma %.6g .. %.6g" %
                  (tag, M, len(rows), d.min().item(), d.max().item(), o[:, 3].min().item(), o[:, 3].max().item()))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g27_render_mlp_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
