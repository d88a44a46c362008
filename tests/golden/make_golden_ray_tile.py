#!/usr/bin/env python3
"""Golden G28: the outputs of the two fused bf16 render kernels on RAY descriptors (mode 1: rays + depths) -- proposal density and fine
(r, g, b, sigma) -- AS THE PARENT OF THE RAY-TILE CHANGE COMPUTED THEM, bit for bit.  The ray-tile instantiations do per-ray work once per
wave instead of once per lane and read a direction encoding that was computed once per ray; every value they feed the MFMAs is produced by the same
expressions, so the kernels must reproduce these numbers exactly, and the descriptors that keep the old kernels (S no multiple of 64, points
in memory) trivially so (tests/test_gpu_ray_tile.py).

Run on an MI355X with the library built from the parent commit (NERF_AMD_LIB may point at it):

    python tests/golden/make_golden_ray_tile.py [OUTPUT.npz]

Inputs are closed-form (the integer hash of nerf_amd.synthetic_weights), so only the outputs are stored: in full for the small ray counts
and on a fixed sample of rows for the large one -- the smallest N at which some persistent workgroup of a 256-CU part runs a third
256-sample tile (1 025 rays at S = 128).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

TAGS = ("small", "he")
N_ROWS = 1536                      # rows kept of a large case
TILE, N_CU = 256, 256
NEAR, FAR = 2.0, 6.0
SEED, RNG_RAY_OFFSET = 0x5EED1234, 77


def big(S: int) -> int:
    """the smallest ray count with more than 2 * N_CU tiles"""
    return (2 * N_CU * TILE) // S + 1


def _cases():
    out = []
    for S in (64, 128, 192):                                   # the ray-tile path: S a multiple of 64
        for N in (1, 2, 5, big(S)):
            out.append(dict(kind="ray", S=S, N=N, zs=S))
    for N in (5, big(128)):                                    # depth rows one longer than S, as the render path passes them
        out.append(dict(kind="ray", S=128, N=N, zs=129))
    for N in (5, big(64)):                                     # proposal pass: depths drawn in the kernel (Philox), uniforms from memory
        out.append(dict(kind="philox", S=64, N=N, zs=64))
        out.append(dict(kind="u", S=64, N=N, zs=64))
    for S in (96, 129):                                        # descriptors that keep the old kernels
        for N in (5, big(S)):
            out.append(dict(kind="ray", S=S, N=N, zs=S))
    for M in (5 * 128, 2 * N_CU * TILE + 37):
        out.append(dict(kind="pts", S=1, N=M, zs=0))
    return out


CASES = _cases()


def key(c) -> str:
    return "%s_S%d_N%d_zs%d" % (c["kind"], c["S"], c["N"], c["zs"])


def has_fine(c) -> bool:
    """the fine kernel takes explicit depths only on the render path: the in-kernel draws are proposal-only cases"""
    return c["kind"] in ("ray", "pts")


def _hash(rows, cols, seed):
    from nerf_amd.synthetic_weights import _hash_uniform
    return _hash_uniform(rows, cols, seed)


def inputs(c):
    """closed-form inputs of a case: rays (N, 6) = origin in [-1, 1)^3 | UNNORMALISED direction in [-1, 1)^3, depths (N, zs) in [NEAR, FAR),
    uniforms (N, S) in [0, 1); mode 0: (M, 6) = position in [-4, 4)^3 | direction in [-1, 1)^3"""
    N, S, zs = c["N"], c["S"], c["zs"]
    if c["kind"] == "pts":
        p = _hash(N, 6, 28000 + N % 1000)
        p[:, :3] *= 8.0
        p[:, 3:] *= 2.0
        return dict(pts=torch.from_numpy(p.astype(np.float32)))
    rays = torch.from_numpy((_hash(N, 6, 28100 + S + N % 1000) * 2.0).astype(np.float32))
    z = torch.from_numpy((NEAR + (FAR - NEAR) * (_hash(N, max(zs, 1), 28200 + S) + 0.5)).astype(np.float32))
    u = torch.from_numpy((_hash(N, S, 28300 + S) + 0.5).astype(np.float32))
    return dict(rays=rays, z=z, u=u)


def kept_rows(M: int) -> np.ndarray:
    """all rows of a small case; of a large one the first 64, the last 256 and a hashed sample of the rest"""
    if M <= N_ROWS:
        return np.arange(M, dtype=np.int64)
    pick = ((_hash(N_ROWS - 320, 1, 2828)[:, 0] + 0.5) * M).astype(np.int64) % M
    return np.unique(np.concatenate((np.arange(64), pick, np.arange(M - 256, M)))).astype(np.int64)


def outputs(ops, pk_prop, pk_mip, c):
    """-> (density (M,), rgbo (M, 4) or None) of the bf16 kernels, fp32 on the host"""
    x = {k: v.cuda() for k, v in inputs(c).items()}
    N, S = c["N"], c["S"]
    dev = torch.device("cuda")
    o = None
    if c["kind"] == "pts":
        d = ops.proposal_forward(pk_prop, ops.BF16, x["pts"][:, :3].contiguous())
        o = ops.mip_forward(pk_mip, ops.BF16, x["pts"])
    else:
        if c["kind"] == "ray":
            sp = ops.samples_rays(x["rays"], S, z=x["z"])
        else:
            z_base = torch.linspace(NEAR, FAR, S).cuda()
            sp = ops.samples_rays(x["rays"], S, z_base=z_base, u=x["u"] if c["kind"] == "u" else None, z_jitter=(FAR - NEAR) / 128.0,
                                  seed=SEED, rng_ray_offset=RNG_RAY_OFFSET)
        d = ops.proposal_forward_samples(pk_prop, ops.BF16, sp, (N, S), dev)
        if has_fine(c):
            o = ops.mip_forward_samples(pk_mip, ops.BF16, ops.samples_rays(x["rays"], S, z=x["z"]), (N, S), dev)
    torch.cuda.synchronize()
    return d.reshape(-1).float().cpu(), (o.reshape(-1, 4).float().cpu() if o is not None else None)


def build_nets(tag: str):
    """-> (packed proposal blob, packed fine blob, the two modules: they own the blobs)"""
    from nerf_amd import addtional, mip_model, ops, synthetic_weights as W
    prop = addtional.ProposalNetwork(10, 256)
    mip = mip_model.MipNeRF(10, 4, 256)
    prop.load_state_dict(W.proposal_state(tag))
    mip.load_state_dict(W.mip_state(tag))
    prop, mip = prop.cuda().eval(), mip.cuda().eval()
    return prop.packed(ops.BF16), mip.packed(ops.BF16), (prop, mip)


def main():
    sys.path.insert(0, ROOT)
    from nerf_amd import ops
    out = {}
    for tag in TAGS:
        pk_prop, pk_mip, _keep = build_nets(tag)
        for c in CASES:
            d, o = outputs(ops, pk_prop, pk_mip, c)
            rows = kept_rows(d.numel())
            out["%s_%s_density" % (tag, key(c))] = d.numpy()[rows].view(np.int32)
            if o is not None:
                out["%s_%s_rgbo" % (tag, key(c))] = o.numpy()[rows].view(np.int32)
            print("%-5s %-24s rows kept %4d of %6d  density %.6g .. %.6g" % (tag, key(c), len(rows), d.numel(), d.min().item(), d.max().item()))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g28_ray_tile_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
