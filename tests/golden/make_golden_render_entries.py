#!/usr/bin/env python3
"""Golden G29: rgb, depth (and in four cases weights) of the four whole-ray render entry points -- ops.render_rays, render_rays_warped,
render_rays_rounds, render_rays_ref -- AS THE COMMIT BEFORE THEY WERE FOLDED INTO ONE PIPELINE COMPUTED THEM, bit for bit, at the smallest
shapes that reach every branch of the entry points: 37 rays (ragged against four waves per workgroup; 5 rays: below the N >= 8 switch of
the direction norm), n_fine 64 (ray-tile kernels) and 40 (fallback), prop_pnum 48 and 64, fp32 and bf16, both spacings, contraction,
integrated PE with and without a caller's norm, white_bkg off, no depth, explicit uniforms and Philox with a ray offset, rays generated
from a camera descriptor, the 128-wide layouts, Ref-NeRF with and without cam_dir.

Run on an MI355X with the library built from that commit:

    python tests/golden/make_golden_render_entries.py [OUTPUT.npz]

Networks are the closed-form weights of tests/weights.py, rays those of a 7 x 7 camera, uniforms a closed-form hash: only outputs are
stored (tests/test_gpu_render_entries.py)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SIDE, RAY0, N = 7, 5, 37                 # rays RAY0 .. RAY0 + N - 1 of the SIDE x SIDE image, raster order
SEED, RNG_OFF = 0x29C0FFEE, 1234
SPACING = {"linear": (2.0, 6.0), "disparity": (0.2, 1000.0)}
IPE_RADIUS = 0.002


def _c(entry, **kw):
    c = dict(entry=entry, prec="fp32", nf=64, P=0, spacing="linear", N=N, contract=False, ipe=None, white=True, depth=True, weights=False, u="philox", off=0,
             gen_rays=False, narrow=False, cam_dir=False)
    c.update(kw)
    if entry == "warped":
        c["spacing"] = "disparity"
    return c


def _cases():
    out = []
    for prec in ("fp32", "bf16"):
        for nf in (40, 64):
            out.append(_c("plain", prec=prec, nf=nf, u="explicit", weights=(prec == "fp32" and nf == 40)))
            out.append(_c("warped", prec=prec, nf=nf, off=RNG_OFF, weights=(prec == "bf16" and nf == 64)))
            # (no bf16 Ref-NeRF case with the normal image: the commit that wrote the fixture did not reproduce that call's own rgb in a second
            # process -- 1 value of 111 -- so there is nothing to pin; fp32 covers cam_dir, bf16 the Ref-NeRF tail without it)
            if (prec, nf) != ("bf16", 64):
                out.append(_c("ref", prec=prec, nf=nf, u="explicit", cam_dir=(nf == 64)))
            for spacing in SPACING:
                out.append(_c("rounds", prec=prec, nf=nf, P=48 if nf == 64 else 64, spacing=spacing, off=RNG_OFF if nf == 40 else 0,
                              weights=(prec == "fp32" and nf == 64)))
    out.append(_c("plain", off=RNG_OFF))                                         # Philox with a ray offset
    out.append(_c("warped", u="explicit"))
    out.append(_c("ref", off=RNG_OFF, cam_dir=True))
    out.append(_c("plain", prec="bf16", contract=True))
    out.append(_c("warped", prec="bf16", contract=True))
    out.append(_c("rounds", prec="bf16", P=64, spacing="disparity", contract=True))
    out.append(_c("ref", prec="bf16", contract=True))
    for ipe in ("own", "given"):                                                 # the entry point's own direction norm | the caller's
        out.append(_c("plain", ipe=ipe))
        out.append(_c("warped", ipe=ipe, prec="bf16"))
        out.append(_c("rounds", ipe=ipe, P=48, spacing="linear" if ipe == "own" else "disparity"))
    out.append(_c("plain", ipe="own", N=5))                                      # N < 8: the one-workgroup norm kernel
    out.append(_c("plain", prec="bf16", white=False))
    out.append(_c("warped", white=False))
    out.append(_c("plain", prec="bf16", depth=False))
    out.append(_c("warped", depth=False))
    out.append(_c("rounds", P=48, spacing="disparity", depth=False))
    out.append(_c("ref", depth=False))
    out.append(_c("plain", gen_rays=True, u="explicit"))                         # rays = None: generated from the camera descriptor
    out.append(_c("plain", gen_rays=True, prec="bf16", off=RNG_OFF))
    out.append(_c("ref", gen_rays=True, u="explicit", cam_dir=True))
    out.append(_c("plain", narrow=True, prec="bf16", u="explicit"))              # NET_PROPOSAL_128 + NET_MIP_128
    out.append(_c("warped", narrow=True))
    out.append(_c("rounds", narrow=True, P=48, prec="bf16"))
    out.append(_c("ref", narrow=True))                                           # NET_PROPOSAL_128 in front of Ref-NeRF
    return out


CASES = _cases()


def key(c) -> str:
    parts = [c["entry"], c["prec"], "nf%d" % c["nf"], c["spacing"], c["u"], "off%d" % c["off"], "N%d" % c["N"]]
    parts += ["P%d" % c["P"]] if c["P"] else []
    parts += [n for n in ("contract", "gen_rays", "narrow", "cam_dir", "weights") if c[n]]
    parts += ["ipe_" + c["ipe"]] if c["ipe"] else []
    parts += [] if c["white"] else ["black"]
    parts += [] if c["depth"] else ["nodepth"]
    return "-".join(parts)


assert len({key(c) for c in CASES}) == len(CASES) and sum(c["weights"] for c in CASES) == 4


def camera():
    """-> (pose (3, 4) on the device, fx, fy)"""
    from nerf_amd import utils
    from oracle import nerf_oracle as O
    fx, fy = utils._focal_xy(O.fov2focal(0.6911112070083618, (SIDE, SIDE)))
    return O.pose_spherical(30.0, -30.0, 4.0)[:3].contiguous().cuda(), float(fx), float(fy)


def build_nets():
    """-> {(kind, narrow): module}: the proposal, MipNeRF and Ref-NeRF networks at the compiled width and at width 128, closed-form weights"""
    import weights as W
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.ref_model import RefNeRF
    nets = {}
    for narrow, hidden in ((False, 256), (True, 128)):
        prop, mip = ProposalNetwork(10, hidden), MipNeRF(10, 4, hidden)
        prop.load_state_dict(W.proposal_state("small", hidden=hidden))
        mip.load_state_dict(W.mip_state("small", hidden=hidden))
        nets["prop", narrow], nets["mip", narrow] = prop.cuda().eval(), mip.cuda().eval()
    ref = RefNeRF(10, 4)
    ref.load_state_dict(W.ref_state("small"))
    nets["ref", False] = nets["ref", True] = ref.cuda().eval()
    return nets


def outputs(ops, nets, c):
    """-> {"rgb", "depth" | None, "weights" | None (Ref-NeRF: the normal image)}: fp32 arrays on the host"""
    import weights as W
    from nerf_amd._lib import Samples
    prec = ops.BF16 if c["prec"] == "bf16" else ops.F32
    near, far = SPACING[c["spacing"]]
    n, nf = c["N"], c["nf"]
    pose, fx, fy = camera()
    rays_all = ops.generate_rays(pose, SIDE, SIDE, fx, fy, pose.device)
    rays = rays_all[RAY0: RAY0 + n].contiguous()
    z_base = torch.linspace(near, far, 64).cuda()
    u1 = u2 = seed = None
    if c["u"] == "explicit":
        u1 = torch.from_numpy((W._hash_uniform(n, 64, 29100 + nf) + 0.5).astype(np.float32)).cuda()
        u2 = torch.from_numpy((W._hash_uniform(n, nf + 1, 29200 + nf) + 0.5).astype(np.float32)).cuda()
    else:
        seed = SEED
    ipe_kw = {}
    if c["ipe"]:
        ipe_kw = dict(ipe_radius=IPE_RADIUS, ipe_dir_norm=ops.dirs_norm(rays_all) if c["ipe"] == "given" else None)
    prop = nets["prop", c["narrow"]].packed(prec)
    fine = nets["ref" if c["entry"] == "ref" else "mip", c["narrow"]]
    fine = fine.packed(prec) if c["entry"] == "ref" else fine.packed(prec, wide=bool(c["ipe"]))
    cam = None
    if c["gen_rays"]:
        cam = Samples()
        cam.H, cam.W, cam.fx, cam.fy = SIDE, SIDE, fx, fy
        for i, v in enumerate(pose.cpu().reshape(-1).tolist()):
            cam.pose[i] = v
    with torch.no_grad():
        if c["entry"] == "plain":
            r = ops.render_rays(prop, fine, prec, None if cam else rays, z_base, u1, u2, nf, near, far, c["white"], want_depth=c["depth"],
                                want_weights=c["weights"], camera=cam, ray_offset=RAY0 if cam else 0, n_rays=n if cam else None, contract=c["contract"],
                                seed=seed, rng_ray_offset=c["off"], **ipe_kw)
        elif c["entry"] == "warped":
            r = ops.render_rays_warped(prop, fine, prec, rays, u1, u2, nf, near, far, c["white"], want_depth=c["depth"], want_weights=c["weights"],
                                       contract=c["contract"], seed=seed, rng_ray_offset=c["off"], spacing=c["spacing"], **ipe_kw)
        elif c["entry"] == "rounds":
            r = ops.render_rays_rounds(prop, fine, prec, rays, z_base, nf, near, far, c["white"], prop_pnum=c["P"], seed=seed, rng_ray_offset=c["off"],
                                       spacing=c["spacing"], contract=c["contract"], want_depth=c["depth"], want_weights=c["weights"], **ipe_kw)
        else:
            r = ops.render_rays_ref(prop, fine, prec, None if cam else rays, z_base, u1, u2, nf, near, far, c["white"], want_depth=c["depth"],
                                    cam_dir=pose[:, 2].contiguous() if c["cam_dir"] else None, camera=cam, ray_offset=RAY0 if cam else 0,
                                    n_rays=n if cam else None, flags=nets["ref", False].kernel_flags, seed=seed, rng_ray_offset=c["off"], contract=c["contract"])
    torch.cuda.synchronize()
    return {name: (t.float().cpu().numpy() if t is not None else None) for name, t in zip(("rgb", "depth", "weights"), r[:3])}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from nerf_amd import ops
    nets = build_nets()
    out = {}
    for c in CASES:
        got = outputs(ops, nets, c)
        assert got["rgb"].shape == (c["N"], 3) and np.isfinite(got["rgb"]).all(), key(c)
        assert (got["depth"] is not None) == c["depth"] and (got["weights"] is not None) == (c["weights"] or c["cam_dir"]), key(c)
        for name, a in got.items():
            if a is not None:
                assert np.isfinite(a).all(), (key(c), name)
                out["%s/%s" % (key(c), name)] = np.ascontiguousarray(a).view(np.int32)
        print("%-70s rgb std %.4f mean %.4f%s" % (key(c), got["rgb"].std(), got["rgb"].mean(),
                                                 "  depth %.4f .. %.4f" % (got["depth"].min(), got["depth"].max()) if c["depth"] else ""))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "g29_render_entries_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays of %d cases, %d bytes" % (path, len(out), len(CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
