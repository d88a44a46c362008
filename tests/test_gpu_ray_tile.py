"""The ray-tile instantiations of the two bf16 render kernels against the kernels they replace.

On a ray descriptor (mode 1) with S a multiple of 64, a wave's 64 samples are one ray: the ray-tile kernels compute the ray index and fetch
the ray once per wave, and the fine kernel reads the direction encoding, computed once per ray by a small kernel that leaves it in the
wave's own block of the output buffer, instead of encoding it per sample and column tile.  Every value that reaches an MFMA comes from the same expressions, so the outputs must be the parent's BIT FOR BIT:
tests/golden/g28_ray_tile_parent.npz was written by tests/golden/make_golden_ray_tile.py on the parent commit.  Descriptors outside the
condition (S in {96, 129}, points in memory) keep the old kernels and must reproduce the same fixture.  The table kernel is compared with
the direction groups that the training forward -- the unchanged per-sample code -- writes to its dump."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_ray_tile", os.path.join(GOLDEN, "make_golden_ray_tile.py"))
G28 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G28)


def _ray_tile(c) -> bool:
    return c["kind"] != "pts" and c["S"] % 64 == 0


RAY_TILE_CASES = [c for c in G28.CASES if _ray_tile(c)]
FALLBACK_CASES = [c for c in G28.CASES if not _ray_tile(c)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import ops
    return ops


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(GOLDEN, "g28_ray_tile_parent.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def nets(ops):
    return {tag: G28.build_nets(tag) for tag in G28.TAGS}


def _check(ops, parent, nets, tag, c):
    pk_prop, pk_mip, _ = nets[tag]
    d, o = G28.outputs(ops, pk_prop, pk_mip, c)
    rows = G28.kept_rows(d.numel())
    name = "%s_%s" % (tag, G28.key(c))
    want_d = parent[name + "_density"]
    bad_d = int((d.numpy()[rows].view(np.int32) != want_d).sum())
    bad_o = n_o = 0
    if G28.has_fine(c):
        want_o = parent[name + "_rgbo"]
        bad_o, n_o = int((o.numpy()[rows].view(np.int32) != want_o).sum()), want_o.size
    print("\n%s: %d of %d density values and %d of %d rgbo values differ from the parent" % (name, bad_d, want_d.size, bad_o, n_o))
    assert np.array_equal(d.numpy()[rows].view(np.int32), want_d)
    if G28.has_fine(c):
        assert np.array_equal(o.numpy()[rows].view(np.int32), parent[name + "_rgbo"])
    # the rows that the fixture does not keep agree with themselves: a second launch gives the same bits everywhere
    d2, o2 = G28.outputs(ops, pk_prop, pk_mip, c)
    assert np.array_equal(d.numpy().view(np.int32), d2.numpy().view(np.int32))
    if o is not None:
        assert np.array_equal(o.numpy().view(np.int32), o2.numpy().view(np.int32))


@pytest.mark.parametrize("c", RAY_TILE_CASES, ids=G28.key)
@pytest.mark.parametrize("tag", G28.TAGS)
def test_ray_tile_kernels_reproduce_the_parent_bit_for_bit(ops, parent, nets, tag, c):
    _check(ops, parent, nets, tag, c)


@pytest.mark.parametrize("c", FALLBACK_CASES, ids=G28.key)
@pytest.mark.parametrize("tag", G28.TAGS)
def test_other_descriptors_keep_the_old_kernels(ops, parent, nets, tag, c):
    _check(ops, parent, nets, tag, c)


@pytest.mark.parametrize("N", (1, 63, 4097))
def test_direction_table_equals_the_per_sample_encoding(ops, nets, N):
    """Row n of the table = [half 0: K groups 0, 1 | half 1: K groups 0, 1] of encode<4, 2>(d / |d|), 16 bytes each.  The training forward
    encodes the direction per sample and writes it to slot 8, K groups 4..5 of its dump (fragment order: 1 KiB per (32-sample subtile, K
    group), 16 bytes per lane, lanes 0..31 = half 0).  With 32 samples per ray, subtile n is ray n."""
    S = 32
    _, pk_mip, _ = nets["small"]
    rays = torch.from_numpy((G28._hash(N, 6, 28400 + N) * 6.0).astype(np.float32)).cuda()            # unnormalised: |d| up to 5
    z = torch.from_numpy((G28.NEAR + 4.0 * (G28._hash(N, S, 28500) + 0.5)).astype(np.float32)).cuda()
    table = ops.direction_table(rays)
    _, dump = ops.mip_forward_train_samples(pk_mip, ops.BF16, ops.samples_rays(rays, S, z=z), (N, S), rays.device)
    torch.cuda.synchronize()
    M = N * S
    n_sub = -(-M // 256) * 8
    layer_stride = n_sub * 16 * 1024
    slot8 = dump[8 * layer_stride:9 * layer_stride].view(n_sub, 16, 64, 16)[:N]                      # (subtile, K group, lane, byte)
    want = torch.stack((slot8[:, 4:6, 0], slot8[:, 4:6, 32]), dim=1)                                 # (ray, half, K group, byte)
    got = table.view(torch.uint8).view(N, 2, 2, 16)
    assert torch.equal(got.cpu(), want.cpu())
    for lane in (1, 31):                                                                             # (every lane of a half holds the same group)
        assert torch.equal(slot8[:, 4:6, lane].cpu(), slot8[:, 4:6, 0].cpu()) and torch.equal(slot8[:, 4:6, 32 + lane].cpu(), slot8[:, 4:6, 32].cpu())
