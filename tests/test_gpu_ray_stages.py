"""The per-ray kernels between the MLP kernels (nerf_amd/csrc/sample_kernels.hip, device_common.h wave_sigma_to_weights), one stage at a time
against the fp64 specifications and per-element bounds of tests/ray_stages_ref.py (derived there, checked on the CPU by
tests/test_ray_stages_ref_host.py): sigma_to_weights, composite, max_blur, get_bounds, weighted_dot_loss and their backwards, called
through nerf_amd.ops.  Every element of every output goes through gate(name, max(err / tol), 1.0); the exact stages through
gate(name, violations, 0).

Row lengths on both sides of every path change: the forward's 2-chunk (S <= 128), 4-chunk (S <= 256) and generic paths (S > 256, or
normals), the backward's 4 / 8 / 16 register chunks (S <= 256 / 512 / ops.BWD_MAX_SAMPLES).  Every ray batch holds the seven input
families of ray_stages_ref.ray_inputs (ray n is of family n % 7).

getBounds: `below` is legal in 0 ... C - 1 (sat has C + 1 entries, en = below + 1 <= C); the reference's torch.gather raises outside that
range and nothing clamps, so neither does the forward kernel (include/nerf_amd.h states the contract).  The cases here hold both ends."""
import ctypes as C

import pytest
import torch

import ray_stages_ref as R
from conftest import gate

pytestmark = pytest.mark.gpu
N = 37
NEAR_FAR = (2.0, 6.0)
# More rays than the launch has waves: blocks_for() in sample_kernels.hip caps the grid at 256 * 8 = 2048 workgroups of WAVES_PER_BLOCK = 4
# waves, one ray per wave and round.  2 * 8192 + 37 rays: every wave takes two rays (the fast paths' next-ray prefetch runs and is consumed),
# waves 0 .. 36 a third one, so the last round is ragged.
N_MANY = 2 * (256 * 8 * 4) + 37


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


@pytest.fixture(scope="module")
def ops():
    from nerf_amd import ops
    return ops


def cu(t):
    return None if t is None else t.cuda()


def _dirs(inp, fl):
    return inp["rays"] if fl["rays6"] else inp["dirs"]


def _tag(S, act, shift, fl=None):
    s = "S=%d act=%d shift=%.1f" % (S, act, shift)
    if fl is not None:
        s += " mn=%d wb=%d nf=%d rays6=%d zx=%d" % (fl["mul_norm"], fl["white_bkg"], fl["near_far"] is not None, fl["rays6"], fl["z_extra"])
    return s


def _composite(ops, inp, fl, act, shift, normals=False, n=N):
    S = inp["sigma"].shape[1]
    nrm = (inp["normal"], inp["cam_dir"]) if normals else (None, None)
    ref = R.composite_ref(inp["rgbo"], inp["z"], _dirs(inp, fl), fl["mul_norm"], fl["white_bkg"], act, shift, fl["near_far"], *nrm)
    rgb, w, depth, nimg = ops.composite(cu(inp["rgbo"]), cu(inp["z"]), cu(_dirs(inp, fl)), fl["mul_norm"], fl["white_bkg"], act, near_far=fl["near_far"],
                                        normal=cu(nrm[0]), cam_dir=cu(nrm[1]), sigma_shift=shift)
    assert (depth is None) == (fl["near_far"] is None) and (nimg is None) == (not normals)
    got = {"rgb": rgb, "w": w, "depth": depth, "normal_img": nimg}
    for name, (want, tol) in ref.items():
        gate("ray_stages composite %s N=%d %s" % (name, n, _tag(S, act, shift, fl)), R.worst(got[name], want, tol), 1.0)


def _upstreams(inp, up):
    return {k: inp[k] if k in up else None for k in ("d_rgb", "d_weights", "d_depth")}


def _composite_backward(ops, inp, fl, act, shift, up, white, n=N):
    S = inp["sigma"].shape[1]
    kw = _upstreams(inp, up)
    want, tol = R.composite_backward_ref(inp["rgbo"], inp["z"], _dirs(inp, fl), fl["mul_norm"], white, act, shift, NEAR_FAR, **kw)
    got = ops.composite_backward(cu(inp["rgbo"]), cu(inp["z"]), cu(_dirs(inp, fl)), fl["mul_norm"], white, act, NEAR_FAR, cu(kw["d_rgb"]), cu(kw["d_weights"]),
                                 cu(kw["d_depth"]), sigma_shift=shift)
    tag = "N=%d %s up=%s wb=%d" % (n, _tag(S, act, shift, fl), "+".join(u[2:] for u in up), white)
    gate("ray_stages composite_backward dsigma " + tag, R.worst(got[..., 3], want[..., 3], tol[..., 3]), 1.0)
    gate("ray_stages composite_backward dc " + tag, R.worst(got[..., :3], want[..., :3], tol[..., :3]), 1.0)


# ------------------------------------------------------------------------------------------------ sigma -> weights, compositing: forward
@pytest.mark.parametrize("S", R.SS)
def test_sigma_to_weights(ops, S):
    for act in (R.ACT_RELU, R.ACT_IDENTITY, R.ACT_SOFTPLUS):
        inp = R.ray_inputs(N, S, act)
        for dirs in (None, inp["dirs"]):
            want, tol = R.sigma_to_weights_ref(inp["sigma"], inp["z"], dirs, act)
            got = ops.sigma_to_weights(cu(inp["sigma"]), cu(inp["z"]), cu(dirs), act)
            gate("ray_stages sigma_to_weights S=%d act=%d dirs=%d" % (S, act, dirs is not None), R.worst(got, want, tol), 1.0)


@pytest.mark.parametrize("S", R.SS)
def test_composite(ops, S):
    for k, (act, shift) in enumerate(R.ACTS):
        fl = R.flags_of(S, k)
        _composite(ops, R.ray_inputs(N, S, act, shift, z_extra=fl["z_extra"]), fl, act, shift)


def test_composite_generic_path_at_300_and_with_normals(ops):
    for k, (act, shift) in enumerate(R.ACTS):
        for S, normals in ((300, False), (64, True)):
            fl = R.flags_of(S, k)
            _composite(ops, R.ray_inputs(N, S, act, shift, z_extra=fl["z_extra"]), fl, act, shift, normals)


@pytest.mark.parametrize("mul_norm", [False, True])
@pytest.mark.parametrize("white_bkg", [False, True])
def test_composite_every_flag_combination(ops, mul_norm, white_bkg):
    """mul_norm x white_bkg x near_far x (N,3) directions / the (N,6) ray table read with stride 6 x z as wide as S / wider (z_stride != S)"""
    S, act, shift = 65, R.ACT_SOFTPLUS, 0.5
    for near_far in (None, NEAR_FAR):
        for rays6 in (False, True):
            for z_extra in (0, 5):
                fl = {"mul_norm": mul_norm, "white_bkg": white_bkg, "near_far": near_far, "rays6": rays6, "z_extra": z_extra}
                _composite(ops, R.ray_inputs(N, S, act, shift, z_extra=z_extra), fl, act, shift)


@pytest.mark.parametrize("S,normals", [(65, False), (129, False), (64, True)], ids=["2-chunk", "4-chunk", "generic"])
def test_composite_more_rays_than_waves(ops, S, normals):
    """N_MANY rays: every wave composites two or three rays, so the fast paths' prefetched second ray is used and the last round is ragged"""
    act, shift = R.ACT_SOFTPLUS, 0.5
    fl = {"mul_norm": True, "white_bkg": True, "near_far": NEAR_FAR, "rays6": True, "z_extra": 3}
    _composite(ops, R.ray_inputs(N_MANY, S, act, shift, z_extra=3), fl, act, shift, normals, n=N_MANY)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("S", R.SS)
def test_composite_backward(ops, S):
    assert max(R.SS) == ops.BWD_MAX_SAMPLES
    for k, (act, shift) in enumerate(R.ACTS):
        fl = R.flags_of(S, k)
        inp = R.ray_inputs(N, S, act, shift, z_extra=fl["z_extra"])
        for up in R.UPSTREAMS:
            _composite_backward(ops, inp, fl, act, shift, up, True if len(up) == 3 else fl["white_bkg"])


@pytest.mark.parametrize("S", R.SS)
def test_sigma_to_weights_backward(ops, S):
    for act in (R.ACT_RELU, R.ACT_IDENTITY, R.ACT_SOFTPLUS):
        inp = R.ray_inputs(N, S, act)
        for dirs in (None, inp["dirs"]):
            want, tol = R.sigma_to_weights_backward_ref(inp["sigma"], inp["z"], dirs, act, inp["d_weights"])
            got = ops.sigma_to_weights_backward(cu(inp["sigma"]), cu(inp["z"]), cu(dirs), act, cu(inp["d_weights"]))
            gate("ray_stages sigma_to_weights_backward S=%d act=%d dirs=%d" % (S, act, dirs is not None), R.worst(got, want, tol), 1.0)


@pytest.mark.parametrize("mul_norm", [False, True])
@pytest.mark.parametrize("white_bkg", [False, True])
def test_composite_backward_every_flag_combination(ops, mul_norm, white_bkg):
    S, act, shift = 65, R.ACT_SOFTPLUS, 0.5
    for rays6 in (False, True):
        for z_extra in (0, 5):
            fl = {"mul_norm": mul_norm, "white_bkg": white_bkg, "near_far": NEAR_FAR, "rays6": rays6, "z_extra": z_extra}
            _composite_backward(ops, R.ray_inputs(N, S, act, shift, z_extra=z_extra), fl, act, shift, R.UPSTREAMS[3], white_bkg)


def test_composite_backward_more_rays_than_waves(ops):
    act, shift = R.ACT_SOFTPLUS, 0.5
    fl = {"mul_norm": True, "white_bkg": True, "near_far": NEAR_FAR, "rays6": True, "z_extra": 3}
    _composite_backward(ops, R.ray_inputs(N_MANY, 65, act, shift, z_extra=3), fl, act, shift, R.UPSTREAMS[3], True, n=N_MANY)


# ------------------------------------------------------------------------------------------------ max-blur
def _blur_inputs(S, integer_g=False):
    gen = torch.Generator().manual_seed(S)
    w = torch.rand(N, S, generator=gen)
    if S >= 2:
        w[:, S // 2] = w[:, S // 2 - 1]                                         # a tie in every row
        w[1] = 0.25                                                             # a row of ties
    g = torch.randint(-8, 9, (N, S), generator=gen).float() if integer_g else torch.randn(N, S, generator=gen)
    return w, g


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257])
def test_max_blur_and_backward(ops, S):
    w, g = _blur_inputs(S)
    for alpha in (0.01, 0.0):
        gate("ray_stages max_blur S=%d alpha=%g" % (S, alpha), R.violations(ops.max_blur(cu(w), alpha), R.max_blur_ref(w, alpha)), 0)
    want, tol = R.max_blur_backward_ref(w, g)
    gate("ray_stages max_blur_backward S=%d" % S, R.worst(ops.max_blur_backward(cu(w), cu(g)), want, tol), 1.0)
    w, g = _blur_inputs(S, integer_g=True)                                      # every sum exact: the tie split to the bit
    gate("ray_stages max_blur_backward exact S=%d" % S, R.violations(ops.max_blur_backward(cu(w), cu(g)), R.max_blur_backward(w, g).float()), 0)


# ------------------------------------------------------------------------------------------------ getBounds
@pytest.mark.parametrize("kind", ["sorted", "unsorted", "constant"])
@pytest.mark.parametrize("C_", [1, 63, 64, 65, 129])
def test_get_bounds_and_backward(ops, C_, kind):
    for K in (2, 65, 130):
        w, below, g = R.bounds_inputs(N, C_, K, kind)
        assert int(below.min()) == 0 and int(below.max()) == C_ - 1            # the legal range 0 ... C - 1, both ends: sat[C] is read
        want, tol = R.get_bounds_ref(w, below)
        gate("ray_stages get_bounds C=%d K=%d %s" % (C_, K, kind), R.worst(ops.get_bounds(cu(w), cu(below)), want, tol), 1.0)
        want, tol = R.get_bounds_backward_ref(below, g, C_)
        gate("ray_stages get_bounds_backward C=%d K=%d %s" % (C_, K, kind), R.worst(ops.get_bounds_backward(cu(below), cu(g), C_), want, tol), 1.0)


# ------------------------------------------------------------------------------------------------ the weighted-dot losses
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 70001])
def test_weighted_dot_loss_and_backward(ops, M, mode):
    w, a, b = R.dot_loss_inputs(M, M + mode)
    scale = 1.0 if mode == 0 else 1.0 / M
    want, tol = R.dot_loss_ref(w, a, b, mode, scale)
    gate("ray_stages weighted_dot_loss M=%d mode=%d" % (M, mode), R.worst(ops.weighted_dot_loss(cu(w), cu(a), cu(b), mode, scale), want, tol), 1.0)
    g = torch.tensor(0.7)
    want, tol = R.dot_loss_backward_ref(g, w, a, b, mode, scale)
    for need in ((True, True, True), (False, True, True), (True, False, True), (True, True, False)):
        got = ops.weighted_dot_loss_backward(cu(g), cu(w), cu(a), cu(b), mode, scale, need=need)
        for name, g_, w_, t_, n_ in zip("wab", got, want, tol, need):
            assert (g_ is None) == (not n_)
            if n_:
                gate("ray_stages weighted_dot_loss_backward d_%s M=%d mode=%d need=%s" % (name, M, mode, "".join("01"[x] for x in need)), R.worst(g_, w_, t_), 1.0)
    w, a, b = R.dot_loss_inputs(M, M + mode, dyadic=True)                       # every product exact
    got = ops.weighted_dot_loss_backward(cu(torch.tensor(0.5)), cu(w), cu(a), cu(b), mode, 0.25)
    want = R.dot_loss_backward(torch.tensor(0.5), w, a, b, mode, 0.25)
    gate("ray_stages weighted_dot_loss_backward exact M=%d mode=%d" % (M, mode), sum(R.violations(g_, w_.float()) for g_, w_ in zip(got, want)), 0)


# ------------------------------------------------------------------------------------------------ overwrite, determinism, empty batches
def _filled(shape, byte, dtype=torch.float32):
    return torch.full(tuple(shape) if len(shape) else (1,), -1 if byte else 0, dtype=torch.int32, device="cuda").view(dtype)


def _every_stage(ops, byte):
    """every stage once at S = 129 / C = 65 / M = 1000 into output buffers pre-filled with `byte`, through the library's entry points (nerf_amd.ops
    allocates its outputs itself) -> the list of outputs"""
    lib, st, p = ops.lib, ops._stream(), (lambda t: C.c_void_p(t.data_ptr()))
    S, act, shift = 129, R.ACT_SOFTPLUS, 0.5
    inp = {k: (v.cuda().contiguous() if torch.is_tensor(v) else v) for k, v in R.ray_inputs(N, S, act, shift, z_extra=3).items()}
    new = lambda *shape: _filled(shape, byte)
    outs = []

    def call(name, *args):
        ops.check(getattr(lib, name)(*args, st), name)

    w, z_s = new(N, S), inp["z"][:, :S].contiguous()
    call("nerf_amd_sigma_to_weights", p(inp["sigma"]), p(z_s), p(inp["dirs"]), N, S, act, p(w))
    outs.append(w)
    for normal in (False, True):
        rgb, wts, depth, nimg = new(N, 3), new(N, S), new(N), new(N)
        call("nerf_amd_composite", p(inp["rgbo"]), p(inp["z"]), S + 3, p(inp["dirs"]), 3, N, S, 3, act, shift, 2.0, 6.0, p(inp["normal"]) if normal else None,
             p(inp["cam_dir"]) if normal else None, p(rgb), p(wts), p(depth), p(nimg) if normal else None)
        outs += [rgb, wts, depth] + ([nimg] if normal else [])
    d_sigma, d_rgbo = new(N, S), new(N, S, 4)
    call("nerf_amd_sigma_to_weights_backward", p(inp["sigma"]), p(z_s), p(inp["dirs"]), N, S, act, p(inp["d_weights"]), p(d_sigma))
    call("nerf_amd_composite_backward", p(inp["rgbo"]), p(inp["z"]), S + 3, p(inp["dirs"]), 3, N, S, 3, act, shift, 2.0, 6.0, p(inp["d_rgb"]), p(inp["d_weights"]),
         p(inp["d_depth"]), p(d_rgbo))
    blur, d_blur = new(N, S), new(N, S)
    call("nerf_amd_max_blur", p(w), N, S, 0.01, p(blur))
    call("nerf_amd_max_blur_backward", p(w), p(inp["d_weights"]), N, S, p(d_blur))
    outs += [d_sigma, d_rgbo, blur, d_blur]
    wp, below, g = (t.cuda() for t in R.bounds_inputs(N, 65, 130, "unsorted"))
    bounds, d_wp = new(N, 129), new(N, 65)
    call("nerf_amd_get_bounds", p(wp), p(below), N, 65, 130, p(bounds))
    call("nerf_amd_get_bounds_backward", p(below), p(g), N, 65, 130, p(d_wp))
    outs += [bounds, d_wp]
    lw, la, lb = (t.cuda() for t in R.dot_loss_inputs(1000, 3))
    gl = torch.tensor([0.7], device="cuda")
    for mode in (0, 1):
        loss, ws, d_w, d_a, d_b = new(1), new(ops.DOT_LOSS_WORKSPACE_FLOATS), new(1000), new(1000, 3), new(1000, 3)
        call("nerf_amd_weighted_dot_loss", p(lw), p(la), p(lb), 1000, mode, 0.5, p(loss), p(ws))
        call("nerf_amd_weighted_dot_loss_backward", p(gl), p(lw), p(la), p(lb), 1000, mode, 0.5, p(d_w), p(d_a), p(d_b))
        outs += [loss, d_w, d_a, d_b]
    torch.cuda.synchronize()
    return [o.view(torch.int32).cpu() for o in outs]


def test_outputs_are_overwritten_and_reproducible(ops):
    """nothing is read before it is written (0x00- and 0xFF-filled output buffers give the same bits) and two calls give the same bits"""
    zero, ones, again = _every_stage(ops, 0x00), _every_stage(ops, 0xFF), _every_stage(ops, 0xFF)
    assert len(zero) == 22
    gate("ray_stages outputs differ between 0x00- and 0xFF-filled buffers", sum(int((a != b).sum()) for a, b in zip(zero, ones)), 0)
    gate("ray_stages outputs differ between two calls", sum(int((a != b).sum()) for a, b in zip(ones, again)), 0)
    assert all(torch.isfinite(o.view(torch.float32)).all() for o in ones)


def test_empty_batches(ops):
    e = lambda *shape: torch.zeros(shape, device="cuda")
    S = 5
    assert ops.sigma_to_weights(e(0, S), e(0, S), e(0, 3), R.ACT_RELU).shape == (0, S)
    rgb, w, depth, nimg = ops.composite(e(0, S, 4), e(0, S), e(0, 3), True, True, R.ACT_RELU, near_far=NEAR_FAR, normal=e(0, S, 3), cam_dir=e(3))
    assert rgb.shape == (0, 3) and w.shape == (0, S) and depth.shape == (0,) and nimg.shape == (0,)
    assert ops.max_blur(e(0, S), 0.01).shape == (0, S) and ops.max_blur_backward(e(0, S), e(0, S)).shape == (0, S)
    below = torch.zeros((0, 4), dtype=torch.int64, device="cuda")
    assert ops.get_bounds(e(0, S), below).shape == (0, 3) and ops.get_bounds_backward(below, e(0, 3), S).shape == (0, S)
    assert ops.sigma_to_weights_backward(e(0, S), e(0, S), None, R.ACT_RELU, e(0, S)).shape == (0, S)
    assert ops.composite_backward(e(0, S, 4), e(0, S), e(0, 6), True, True, R.ACT_SOFTPLUS, NEAR_FAR, e(0, 3), e(0, S), e(0)).shape == (0, S, 4)
    loss = ops.weighted_dot_loss(e(0), e(0, 3), e(0, 3), 0, 1.0)
    assert loss.shape == () and float(loss) == 0.0
    d_w, d_a, d_b = ops.weighted_dot_loss_backward(e(1).reshape(()), e(0), e(0, 3), e(0, 3), 1, 1.0)
    assert d_w.shape == (0,) and d_a.shape == (0, 3) and d_b.shape == (0, 3)
    torch.cuda.synchronize()
