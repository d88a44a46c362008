"""The sampling side of nerf_amd/csrc/sample_kernels.hip -- wave_inverse_sample behind inverse_sample_kernel (both modes) and the fused
resampling kernels, and the depth draws stratified_points, warped_stratified, warp_depths (both directions), length2pts -- against the fp64
specification and per-element bounds of tests/sampling_ref.py (derived there, checked on the CPU by tests/test_sampling_ref_host.py, which
runs the SAME check functions over a torch-fp32 emulation).  Every element of every output goes through gate(name, max(err / tol), 1.0);
`below`, `above` and the order of the sorted output are discrete and go through gate(name, violations, 0).

Row lengths nw: 1, 3 (shortest), 7 (scalar normaliser), 8, 15 (vector + tail), 32 (four-way interleave), 64 (one scan chunk), 65, 128, 129
(carry), 254 / 255 (largest legal).  Sample counts on both sides of the 192-sample search chunk.  A handful of rays per call: ray n holds
weight family n % 3 (benign, all zero, one sample with all the mass) and bin family n // 3 (metric, s-space, log-spaced, equal neighbours,
descending, mixed sign); the uniforms are random, all in one bucket of the sort, EVERY interior CDF edge with its two fp32 neighbours, and
the special values 0, 1 - 2^-24, 1, the smallest subnormal, below 0 and above 1.  test_constructed_cross_bucket_rows holds the rows at
which the raw samples descend across a boundary of the sort's buckets."""
import pytest
import torch

import sampling_ref as S
from conftest import gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def cu(t):
    return t.cuda().contiguous()


class Device:
    """sampling_ref.Emulation's interface over nerf_amd.ops"""

    def __init__(self):
        from nerf_amd import ops
        self.ops = ops

    def inverse(self, w, z, u, mode, sort):
        if mode == 0:
            v, below = self.ops.inverse_sample(cu(w), cu(z), cu(u), bool(sort))
            return v.cpu(), below.cpu(), None
        assert not sort
        v, below, above = self.ops.sample_pdf(cu(z), cu(w), cu(u))
        return v.cpu(), below.cpu(), above.cpu()

    def resample(self, inp, u, warped):
        K = u.shape[1]
        if warped:
            zf, sf, below, w = self.ops.warped_resample(cu(inp["density"]), cu(inp["x"]), cu(inp["rays"]), cu(u), *S.NEAR_FAR_WARP)
            return sf.cpu(), below.cpu(), w.cpu(), zf.cpu()
        zf, below, w, _ = self.ops.resample(cu(inp["density"]), cu(inp["x"]), None, None, 0.0, cu(inp["rays"]), cu(u), K, want_below=True, want_w=True)
        return zf.cpu(), below.cpu(), w.cpu(), None

    def stratified(self, rays, z_base, u, jitter):
        z, pts = self.ops.stratified_points(cu(rays), cu(z_base), cu(u), jitter)
        return z.cpu(), pts.cpu()

    def warped_stratified(self, rays, u, near, far):
        return tuple(t.cpu() for t in self.ops.warped_stratified(cu(rays), cu(u), near, far))

    def warp(self, s, near, far, rays):
        z, pts = self.ops.warp_depths(cu(s), near, far, cu(rays))
        return z.cpu(), pts.cpu()

    def unwarp(self, z, near, far):
        return self.ops.warp_depths(cu(z), near, far, inverse=True)[0].cpu()

    def length2pts(self, rays, z):
        return self.ops.length2pts(cu(rays), cu(z)).cpu()


@pytest.fixture(scope="module")
def dev():
    return Device()


def _gates(items):
    failed = []
    for name, value, limit in items:            # every figure goes on record before the first assertion fails
        try:
            gate(name, value, limit)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("nw,mode", S.CASES)
def test_inverse_sampling_row_lengths(dev, nw, mode):
    _gates(S.inverse_case_gates(dev, nw, mode))


@pytest.mark.parametrize("K", S.KS)
def test_inverse_sampling_sample_counts(dev, K):
    _gates(S.sample_count_gates(dev, K))


def test_constructed_cross_bucket_rows(dev):
    """ascending bins, ascending uniforms on the two sides of a bucket boundary, DESCENDING raw samples: the output must still be sorted by value"""
    _gates(S.cross_bucket_gates(dev))


@pytest.mark.parametrize("C,K", S.FUSED_SHAPES)
def test_fused_resample(dev, C, K):
    _gates(S.fused_gates(dev, C, K, False))


def test_fused_warped_resample(dev):
    _gates(S.fused_gates(dev, *S.WARPED_SHAPE, True))


@pytest.mark.parametrize("Sn", S.DRAW_SIZES)
def test_depth_draws(dev, Sn):
    _gates(S.draw_gates(dev, Sn))
