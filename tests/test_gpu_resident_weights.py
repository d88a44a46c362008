"""The bf16 render kernels with part of their weight stream resident in LDS (mlp_core.h ResidentSet) against the kernels they replace.

Residency changes where an A fragment is read from -- a fixed LDS address instead of a ring slot -- and nothing about the MFMAs or their
operands, so the outputs must be the parent's BIT FOR BIT: tests/golden/g27_render_mlp_parent.npz was written by
tests/golden/make_golden_render_mlp.py on the parent commit.  Sizes: 1, 255, 257 (ragged tiles) and 2 * 256 * 256 + 37 (a third tile per
persistent workgroup on a 256-CU part: the ring wraps across tiles with the resident area in place)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_golden_render_mlp", os.path.join(GOLDEN, "make_golden_render_mlp.py"))
G27 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G27)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    return nerf_amd


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(GOLDEN, "g27_render_mlp_parent.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def nets(pkg):
    return {tag: G27.build_nets(tag) for tag in G27.TAGS}


@pytest.mark.parametrize("M", G27.SIZES)
@pytest.mark.parametrize("tag", G27.TAGS)
def test_render_mlps_reproduce_the_parent_bit_for_bit(pkg, parent, nets, tag, M):
    prop, mip = nets[tag]
    d, o = G27.render_mlp_outputs(pkg, prop, mip, M)
    rows = parent["rows_%d" % M]
    assert np.array_equal(rows, G27.kept_rows(M))
    got_d, got_o = d.numpy()[rows].view(np.int32), o.numpy()[rows].view(np.int32)
    want_d, want_o = parent["%s_%d_density" % (tag, M)], parent["%s_%d_rgbo" % (tag, M)]
    bad_d, bad_o = int((got_d != want_d).sum()), int((got_o != want_o).sum())
    print("\n%s M=%d: %d of %d density values and %d of %d rgbo values differ from the parent" % (tag, M, bad_d, want_d.size, bad_o, want_o.size))
    assert bad_d == 0 and bad_o == 0
    # ... and the rows that the fixture does not keep agree with themselves: a second launch gives the same bits everywhere
    d2, o2 = G27.render_mlp_outputs(pkg, prop, mip, M)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(o.view(torch.int32), o2.view(torch.int32))


@pytest.mark.parametrize("tag", G27.TAGS)
def test_repack_after_update_equals_a_fresh_module(pkg, nets, tag):
    """In-place updates of resident AND streamed layers followed by the repack: the same bits as a module freshly built from the updated
    parameters (nothing the kernels read survives from the old pack)."""
    M = 257
    prop, mip = G27.build_nets(tag)
    G27.render_mlp_outputs(pkg, prop, mip, M)                                    # packs the original weights
    with torch.no_grad():
        for lin, k in ((prop.layers[0], 1.25), (prop.layers[4], 0.75), (prop.layers[6], 1.5), (prop.layers[8], 0.5)):
            lin.weight.mul_(k); lin.bias.add_(0.125)
        for lin, k in ((mip.lin_block1[0], 1.25), (mip.lin_block1[4], 0.75), (mip.rgb_layer[0], 1.5), (mip.rgb_layer[2], 0.5), (mip.opacity_head[0], 2.0)):
            lin.weight.mul_(k); lin.bias.add_(0.125)
    d, o = G27.render_mlp_outputs(pkg, prop, mip, M)
    prop2, mip2 = G27.build_nets(tag)
    prop2.load_state_dict(prop.state_dict()); mip2.load_state_dict(mip.state_dict())
    d2, o2 = G27.render_mlp_outputs(pkg, prop2, mip2, M)
    d0, o0 = G27.render_mlp_outputs(pkg, *nets[tag], M)
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32)) and torch.equal(o.view(torch.int32), o2.view(torch.int32))
    assert not torch.equal(d, d0) and not torch.equal(o, o0)                    # (the update did change the outputs)
