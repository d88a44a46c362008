"""The four whole-ray render entry points against their own outputs from before they were folded into one pipeline.

tests/golden/g29_render_entries_parent.npz was written by tests/golden/make_golden_render_entries.py on the parent commit, on an MI355X: rgb,
depth and (in four cases) weights of ops.render_rays, render_rays_warped, render_rays_rounds and render_rays_ref at the smallest shapes that
reach every branch of the entry points.  The fold changes no kernel and no launch, so every array must come out BIT FOR BIT (compared as
int32)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_render_entries", os.path.join(GOLDEN, "make_golden_render_entries.py"))
G29 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G29)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nerf_amd import ops
    return ops


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(GOLDEN, "g29_render_entries_parent.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def nets(ops):
    return G29.build_nets()


def test_the_fixture_holds_exactly_the_cases(parent):
    want = set()
    for c in G29.CASES:
        want.add(G29.key(c) + "/rgb")
        if c["depth"]:
            want.add(G29.key(c) + "/depth")
        if c["weights"] or c["cam_dir"]:
            want.add(G29.key(c) + "/weights")
    assert set(parent) == want
    assert sum(c["weights"] for c in G29.CASES) == 4 and {c["entry"] for c in G29.CASES} == {"plain", "warped", "rounds", "ref"}


@pytest.mark.parametrize("via,c", [(via, c) for via in ("request", "abi") for c in G29.CASES],
                         ids=[G29.key(c) + suffix for suffix in ("", "-abi") for c in G29.CASES])
def test_entry_points_reproduce_the_parent_bit_for_bit(ops, parent, nets, c, via):
    """via "request": the package, which renders through nerf_amd_render (ids as before: the case alone); "abi": the argument-list C entry
    points, called directly (abi_render)."""
    import abi_render
    got = G29.outputs(ops if via == "request" else abi_render, nets, c)
    name = G29.key(c)
    for what, a in got.items():
        if a is None:
            assert name + "/" + what not in parent
            continue
        want = parent[name + "/" + what]
        bits = np.ascontiguousarray(a).view(np.int32)
        print("\n%s/%s: %d of %d values differ from the parent" % (name, what, int((bits != want).sum()) if bits.shape == want.shape else -1, want.size))
        assert bits.shape == want.shape and np.array_equal(bits, want), (name, what)
