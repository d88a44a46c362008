"""Elastic tiles: the bf16 render instantiations of proposal_kernel and mip_kernel hand their tiles out through an atomic counter
(mlp_kernels.hip TileQueue) instead of a static share per workgroup.  A tile's results depend on its index alone, so the outputs must be
those of the static loop BIT FOR BIT: every case is compared with the same call in a process that loads the same sources built with
-DMLP_ELASTIC=0 (nerf_amd/ablate/libnerf_amd_STATIC_TILES.so, built next to the library; NERF_AMD_LIB names it), computed once per module.

Sizes, with CU the device's compute units (= persistent workgroups) and 256-sample tiles: M = 64 (fewer tiles than workgroups), 256 (CU - 1),
256 CU (exactly one tile each: nothing is handed out), 256 (CU + 1) (exactly one dynamic tile), 2 * 256 * CU + 64 (a workgroup takes several;
the last tile is a quarter full).  Each as a ray descriptor with S = 64 (the ray-tile instantiations, PBF16WR) and as points in memory (the
PBF16W instantiations).  Then the counter's life: launches back to back on one stream (zeroed in stream order in between), launches on two
streams at once (a counter per stream), and 20 repeats of the largest case (no tile lost, none done twice: a lost tile leaves the poison
of the output buffer, a repeated one is invisible in the values but costs the count that another tile needed)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
STATIC_LIB = os.path.join(ROOT, "nerf_amd", "ablate", "libnerf_amd_STATIC_TILES.so")

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_ray_tile", os.path.join(GOLDEN, "make_golden_ray_tile.py"))
G28 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G28)

TILE, S = 256, 64
SIZES = {"one_wave": lambda cu: 64, "cu_minus_1": lambda cu: TILE * (cu - 1), "cu": lambda cu: TILE * cu, "cu_plus_1": lambda cu: TILE * (cu + 1),
         "two_cu_and_a_quarter": lambda cu: 2 * TILE * cu + 64}
KINDS = ("ray", "pts")
BIG = "two_cu_and_a_quarter"


def case_of(kind, M):
    return dict(kind="ray", S=S, N=M // S, zs=S) if kind == "ray" else dict(kind="pts", S=1, N=M, zs=0)


def device_inputs(kind, M):
    x = {k: v.cuda() for k, v in G28.inputs(case_of(kind, M)).items()}
    if kind == "pts":
        x["pts3"] = x["pts"][:, :3].contiguous()                 # the proposal kernel's (M, 3) positions
    return x


def launch(ops, nets, kind, x, M):
    """-> (density (M,), rgbo (M, 4)) on the device, on the current stream, not synchronised; the outputs start from a poison value"""
    import ctypes as C
    pk_prop, pk_mip, _ = nets
    d = torch.full((M,), float("nan"), dtype=torch.float32, device="cuda")          # (a tile that nobody computes stays NaN; torch.empty could
    o = torch.full((M, 4), float("nan"), dtype=torch.float32, device="cuda")        #  hand back an earlier launch's correct block)
    if kind == "pts":
        sp, sf = ops._samples_pts(x["pts3"], 3), ops._samples_pts(x["pts"], 6)
    else:
        sp = sf = ops.samples_rays(x["rays"], S, z=x["z"])
    ops.check(ops.lib.nerf_amd_proposal_forward(ops._ptr(pk_prop), ops.BF16, C.byref(sp), ops._ptr(d), ops._stream()), "nerf_amd_proposal_forward")
    ops.check(ops.lib.nerf_amd_mip_forward(ops._ptr(pk_mip), ops.BF16, C.byref(sf), ops._ptr(o), ops._stream()), "nerf_amd_mip_forward")
    return d, o


def bits(t):
    return t.reshape(-1).view(torch.int32)


def _worker(path):
    """the reference process: every case under the library that NERF_AMD_LIB names"""
    sys.path.insert(0, ROOT)
    from nerf_amd import _lib, ops
    assert os.path.samefile(_lib.LIB_PATH, STATIC_LIB), _lib.LIB_PATH
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    nets = G28.build_nets("small")
    out = {}
    for kind in KINDS:
        for name, size in SIZES.items():
            M = size(cu)
            d, o = launch(ops, nets, kind, device_inputs(kind, M), M)
            torch.cuda.synchronize()
            out["%s_%s_density" % (kind, name)] = bits(d).cpu().numpy()
            out["%s_%s_rgbo" % (kind, name)] = bits(o).cpu().numpy()
    np.savez(path, cu=np.int64(cu), **out)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import ops
    return ops


@pytest.fixture(scope="module")
def cu(ops):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def nets(ops):
    return G28.build_nets("small")


@pytest.fixture(scope="module")
def static(ops, cu, tmp_path_factory):
    """the static loop's outputs of every case, as int32 bit patterns on the device"""
    assert os.path.exists(STATIC_LIB), "%s is missing: `make -C nerf_amd/csrc` builds it with the library" % STATIC_LIB
    path = str(tmp_path_factory.mktemp("elastic") / "static.npz")
    env = dict(os.environ, NERF_AMD_LIB=STATIC_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "the reference process failed:\n%s\n%s" % (r.stdout[-2000:], r.stderr[-4000:])
    with np.load(path) as f:
        assert int(f["cu"]) == cu
        return {k: torch.from_numpy(f[k]).cuda() for k in f.files if k != "cu"}


def _same(static, kind, name, d, o, what=""):
    for tag, got in (("density", d), ("rgbo", o)):
        want = static["%s_%s_%s" % (kind, name, tag)]
        bad = int((bits(got) != want).sum().item())
        print("%s %s %s%s: %d of %d values differ from the static loop" % (kind, name, tag, what, bad, want.numel()))
        assert bad == 0, "%s %s %s%s: %d of %d values differ from the static loop" % (kind, name, tag, what, bad, want.numel())


@pytest.mark.parametrize("name", list(SIZES))
@pytest.mark.parametrize("kind", KINDS)
def test_outputs_equal_the_static_loop_bit_for_bit(ops, cu, nets, static, kind, name):
    M = SIZES[name](cu)
    d, o = launch(ops, nets, kind, device_inputs(kind, M), M)
    torch.cuda.synchronize()
    _same(static, kind, name, d, o)


@pytest.mark.parametrize("kind", KINDS)
def test_back_to_back_launches_on_one_stream(ops, cu, nets, static, kind):
    """no synchronisation in between: the counter is zeroed in stream order ahead of each launch that hands tiles out"""
    order = (BIG, "cu_plus_1", BIG, "one_wave", "cu_plus_1")
    xs = {name: device_inputs(kind, SIZES[name](cu)) for name in set(order)}
    torch.cuda.synchronize()
    outs = [launch(ops, nets, kind, xs[name], SIZES[name](cu)) for name in order]
    torch.cuda.synchronize()
    for i, (name, (d, o)) in enumerate(zip(order, outs)):
        _same(static, kind, name, d, o, " (launch %d of %d)" % (i + 1, len(order)))


@pytest.mark.parametrize("kind", KINDS)
def test_launches_on_two_streams_at_once(ops, cu, nets, static, kind):
    """two streams, four launch pairs each, enqueued alternately: launches in flight on different streams count on different counters"""
    names = (BIG, "cu_plus_1")
    xs = {name: device_inputs(kind, SIZES[name](cu)) for name in names}
    torch.cuda.synchronize()
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    outs = []
    for rep in range(4):
        for k, st in enumerate(streams):
            name = names[(k + rep) % 2]
            with torch.cuda.stream(st):
                outs.append((name, k, launch(ops, nets, kind, xs[name], SIZES[name](cu))))
    torch.cuda.synchronize()
    for i, (name, k, (d, o)) in enumerate(outs):
        _same(static, kind, name, d, o, " (stream %d, launch %d)" % (k, i // 2 + 1))


@pytest.mark.parametrize("kind", KINDS)
def test_twenty_repeats_lose_no_tile(ops, cu, nets, static, kind):
    M = SIZES[BIG](cu)
    x = device_inputs(kind, M)
    torch.cuda.synchronize()
    outs = [launch(ops, nets, kind, x, M) for _ in range(20)]
    torch.cuda.synchronize()
    for i, (d, o) in enumerate(outs):
        _same(static, kind, BIG, d, o, " (repeat %d)" % (i + 1))


if __name__ == "__main__":
    _worker(sys.argv[1])
