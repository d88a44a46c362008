"""The yardstick of tests/test_gpu_ray_stages.py, tested on the CPU (tests/ray_stages_ref.py).

  * the fp64 specifications equal the oracle's (oracle/nerf_oracle.py) on the golden inputs g05, g10 and g14: to 1e-12 when the oracle is run
    in fp64 on the same inputs, and to fp32 rounding against the recorded fp32 results;
  * the hand-derived adjoint behind the backward bounds equals torch.autograd in fp64;
  * a torch-fp32 evaluation of every stage -- forward, autograd backward and the kernel's own backward formula -- stays inside its bound on
    every element of every input family, row length, activation and flag combination the GPU module runs; its worst err / tol goes on
    record through conftest.gate;
  * the bounds bite: each single-term mutation of that fp32 evaluation is reported with a ratio > 1 by the comparator the GPU module uses;
  * the gate the old tests use, 2e-5 * max(1, max |want|), lets one of those mutations through.

SLACK.  Worst err / tol of the fp32 emulation over all of these cases (the gates print the current figures), and so the factor by which
each bound exceeds what an honest fp32 evaluation needs:

    weights 0.89 (1.1x)      rgb 0.24 (4x)           depth 0.33 (3x)          normal image 0.61 (1.6x)
    dL/dsigma 0.91 (1.1x)    dL/dc 0.81 (1.2x)       sigma_to_weights and its backward 0.82 / 0.87 (1.2x)
    getBounds 0.93 (1.1x)    its backward 0.99 (1.0x)    max-blur backward 0.43 (2.3x)    dot losses 0.15 (7x), their backward 0.78 (1.3x)

Every factor is below 8.  The element-wise stages sit close to 1 because their bounds are a handful of roundings and the worst element of a
few thousand meets one of them almost in full: a depth just above a power of two is rounded by nearly u |zn| on both sides of the
subtraction delta = zn_{s+1} - zn_s, and sigma = 400 multiplies that into m, T and everything behind the sample.  The sums are looser: rgb,
depth and the dot losses charge every term its full u with the same sign and the longest chain of additions (D u sum |t|), while roundings
are at most u / 2 and add up like a random walk; expf, log1pf, sqrtf and the division are charged the device library's documented
3 / 2 / 3 / 2.5 ulp while the host library the emulation runs on is within 1 ulp."""
import pytest
import torch
import torch.nn.functional as F

import ray_stages_ref as R
import torch_spec as TS
import weights as W
from conftest import gate, max_abs
from oracle import nerf_oracle as O

F32, F64 = torch.float32, torch.float64
NEAR, FAR = 2.0, 6.0
N = 37


def _close(got, want, rel=1e-12):
    return float((got.double() - want.double()).abs().max()) <= rel * max(1.0, float(want.double().abs().max()))


# ------------------------------------------------------------------------------------------------ the specifications against the oracle
def test_weights_spec_equals_the_oracle_on_g05(golden):
    g = golden("g05_weights")
    s, z, d = g["sigma"], g["z"], g["dirs"]
    for dirs, act, key, fn in ((d, R.ACT_RELU, "w_prop", F.relu), (None, R.ACT_RELU, "w_nerf", F.relu)):
        want, tol = R.sigma_to_weights_ref(s, z, dirs, act)
        assert _close(want, O.sigma_to_weights(s.double(), z.double(), None if dirs is None else dirs.double(), fn))
        assert max_abs(want, g[key]) <= 1e-6
        assert _close(want, TS.weights_expr(s.double(), z.double() * (1.0 if dirs is None else dirs.double().norm(dim=-1, keepdim=True)), act))
    want, _ = R.sigma_to_weights_ref(s.abs(), z, None, R.ACT_IDENTITY)
    assert _close(want, O.sigma_to_weights(s.double(), z.double(), None, lambda t: t.abs())) and max_abs(want, g["w_nerf_id"]) <= 1e-6


def test_composite_spec_equals_the_oracle_on_g10(golden):
    g = golden("g10_composite")
    for wb in (False, True):
        for mn in (False, True):
            ref = R.composite_ref(g["rgbo"], g["z"], g["dirs"], mn, wb, R.ACT_RELU, 0.0, (NEAR, FAR), g["normal"], g["cam_z"])
            rgb, w, ex = O.composite(g["rgbo"].double(), g["z"].double(), g["dirs"].double(), mul_norm=mn, white_bkg=wb, render_depth=(NEAR, FAR),
                                     normal_info=(g["normal"].double(), g["cam_z"].double()))
            for name, o in (("rgb", rgb), ("w", w), ("depth", ex["depth_img"]), ("normal_img", ex["normal_img"])):
                assert _close(ref[name][0], o), (wb, mn, name)
            k = "wb%d_mn%d_" % (wb, mn)
            for name, key in (("rgb", "rgb"), ("w", "w"), ("depth", "depth"), ("normal_img", "normal")):
                assert max_abs(ref[name][0], g[k + key]) <= 2e-6, (wb, mn, name)
    ref = R.composite_ref(g["rgbo"], g["z"], g["dirs"], True, False, R.ACT_SOFTPLUS)
    rgb, w, _ = O.composite(g["rgbo"].double(), g["z"].double(), g["dirs"].double(), density_act=F.softplus)
    assert _close(ref["rgb"][0], rgb) and _close(ref["w"][0], w)
    assert max_abs(ref["rgb"][0], g["softplus_rgb"]) <= 2e-6 and max_abs(ref["w"][0], g["softplus_w"]) <= 2e-6


def test_bounds_and_loss_specs_equal_the_oracle_on_g14(golden):
    g = golden("g14_train_step")
    prop_sd = W.proposal_state("small")
    rays, z_c = g["rays"], g["z_coarse"]
    with torch.no_grad():
        dens = F.softplus(O.proposal_forward(prop_sd, rays[:, None, :3] + rays[:, None, 3:] * z_c[:, :, None]))
        pw = O.max_blur(O.sigma_to_weights(dens, z_c, rays[:, 3:]), 0.01)
    assert R.violations(R.max_blur_ref(O.sigma_to_weights(dens, z_c, rays[:, 3:]), 0.01), pw) == 0
    want, tol = R.get_bounds_ref(pw, g["below"])
    assert _close(want, O.get_bounds(pw.double(), g["below"])) and max_abs(want, g["bounds"]) <= 1e-5
    assert R.worst(O.get_bounds(pw, g["below"]), want, tol * 64) <= 1.0              # (the oracle's fp32 cumsum is sequential)
    gb = torch.randn(32, 64, generator=torch.Generator().manual_seed(3))
    x = pw.double().requires_grad_(True)
    auto, = torch.autograd.grad(TS.bounds_expr(x, g["below"]).float().double(), x, gb.double())
    assert _close(R.get_bounds_backward_ref(g["below"], gb, 32)[0], auto)
    # the dot losses on the recorded weights: WeightedNormalLoss is a plain sum, BackFaceLoss a mean
    wts = g["weights"]
    gen = torch.Generator().manual_seed(5)
    a, b = F.normalize(torch.randn(32, 64, 3, generator=gen), dim=-1), F.normalize(torch.randn(32, 64, 3, generator=gen), dim=-1)
    assert _close(R.dot_loss_ref(wts, a, b, 0, 1.0)[0], O.weighted_normal_loss(wts.double(), a.double(), b.double()))
    assert _close(R.dot_loss_ref(wts, a, b, 1, 1.0 / wts.numel())[0], O.back_face_loss(wts.double(), a.double(), b.double()), 1e-9)
    for mode, fn, scale in ((0, O.weighted_normal_loss, 1.0), (1, O.back_face_loss, 1.0 / wts.numel())):
        leaves = [t.double().requires_grad_(True) for t in (wts, a, b)]
        auto = torch.autograd.grad(fn(*leaves) * 0.75, leaves)
        mine, _ = R.dot_loss_backward_ref(torch.tensor(0.75), wts, a, b, mode, scale)
        for m_, a_ in zip(mine, auto):
            assert _close(m_, a_, 1e-9), mode


@pytest.mark.parametrize("act,shift", R.ACTS)
def test_adjoint_formula_equals_autograd_in_fp64(act, shift):
    """the suffix-sum adjoint the backward bounds are derived from is the gradient"""
    for S in (1, 2, 65, 257):
        inp = R.ray_inputs(N, S, act, shift)
        ok = inp["family"] != R.FAMILIES.index("opaque_prefix")             # (cumprod's autograd divides by the product: 0 / 0 in fp64 only far below fp32's range)
        for up in R.UPSTREAMS:
            kw = {k: inp[k] if k in up else None for k in ("d_rgb", "d_weights", "d_depth")}
            for mn, wb in ((True, True), (False, False)):
                a = R.composite_backward_autograd(inp["rgbo"], inp["z"], inp["dirs"], mn, wb, act, shift, (NEAR, FAR), **kw)
                f = R.composite_backward_formula(inp["rgbo"], inp["z"], inp["dirs"], mn, wb, act, shift, (NEAR, FAR), **kw)
                assert torch.isfinite(a).all() and torch.isfinite(f).all()
                assert float((a - f)[ok].abs().max()) <= 1e-11 * max(1.0, float(f.abs().max())), (S, up, mn, wb)


# ------------------------------------------------------------------------------------------------ the fp32 emulation inside every bound
RECORD = {}


def _note(name, value):
    RECORD[name] = max(RECORD.get(name, 0.0), value)
    return value


@pytest.fixture(autouse=True)
def _slack_on_record():
    """the worst err / tol the fp32 emulation reached in a test, per stage, through conftest.gate"""
    RECORD.clear()
    yield
    for name, value in sorted(RECORD.items()):
        gate("ray_stages_ref fp32 emulation: " + name, value, 1.0)


def _dirs(inp, fl):
    return inp["rays"] if fl["rays6"] else inp["dirs"]


def _forward_case(S, k, act, shift, normals):
    fl = R.flags_of(S, k)
    inp = R.ray_inputs(N, S, act, shift, z_extra=fl["z_extra"])
    nrm = (inp["normal"], inp["cam_dir"]) if normals else (None, None)
    ref = R.composite_ref(inp["rgbo"], inp["z"], _dirs(inp, fl), fl["mul_norm"], fl["white_bkg"], act, shift, fl["near_far"], *nrm)
    emu = R.evaluate(inp["rgbo"], inp["z"], _dirs(inp, fl), fl["mul_norm"], fl["white_bkg"], act, shift, fl["near_far"], *nrm)
    for name, (want, tol) in ref.items():
        assert _note("composite " + name, R.worst(emu[name], want, tol)) <= 1.0, (S, act, shift, fl, name)


@pytest.mark.parametrize("S", R.SS)
def test_fp32_emulation_of_the_forward_stays_inside_the_bounds(S):
    for k, (act, shift) in enumerate(R.ACTS):
        _forward_case(S, k, act, shift, normals=False)
        inp = R.ray_inputs(N, S, act)
        for dirs in (None, inp["dirs"]):
            want, tol = R.sigma_to_weights_ref(inp["sigma"], inp["z"], dirs, act)
            emu = R.chain(inp["sigma"], inp["z"], dirs, dirs is not None, act, 0.0)["w"]
            assert _note("sigma_to_weights", R.worst(emu, want, tol)) <= 1.0, (S, act, dirs is None)


def test_fp32_emulation_of_the_forward_with_normals_and_at_300():
    for k, (act, shift) in enumerate(R.ACTS):
        _forward_case(64, k, act, shift, normals=True)
        _forward_case(300, k, act, shift, normals=False)


N_MANY = 2 * 8192 + 37                      # test_gpu_ray_stages.N_MANY: more rays than the launch has waves


@pytest.mark.parametrize("S,normals", [(65, False), (129, False), (64, True)])
def test_fp32_emulation_of_the_many_ray_cases(S, normals):
    act, shift = R.ACT_SOFTPLUS, 0.5
    inp = R.ray_inputs(N_MANY, S, act, shift, z_extra=3)
    nrm = (inp["normal"], inp["cam_dir"]) if normals else (None, None)
    ref = R.composite_ref(inp["rgbo"], inp["z"], inp["rays"], True, True, act, shift, (NEAR, FAR), *nrm)
    emu = R.evaluate(inp["rgbo"], inp["z"], inp["rays"], True, True, act, shift, (NEAR, FAR), *nrm)
    for name, (want, tol) in ref.items():
        assert _note("composite " + name, R.worst(emu[name], want, tol)) <= 1.0, name
    if S == 65:
        args = (inp["rgbo"], inp["z"], inp["rays"], True, True, act, shift, (NEAR, FAR), inp["d_rgb"], inp["d_weights"], inp["d_depth"])
        want, tol = R.composite_backward_ref(*args)
        got = R.composite_backward_formula(*args, dt=F32)
        assert _note("composite_backward dsigma", R.worst(got[..., 3], want[..., 3], tol[..., 3])) <= 1.0
        assert _note("composite_backward dc", R.worst(got[..., :3], want[..., :3], tol[..., :3])) <= 1.0


@pytest.mark.parametrize("S", R.SS)
def test_fp32_emulation_of_the_backward_stays_inside_the_bounds(S):
    for k, (act, shift) in enumerate(R.ACTS):
        fl = R.flags_of(S, k)
        inp = R.ray_inputs(N, S, act, shift, z_extra=fl["z_extra"])
        for j, up in enumerate(R.UPSTREAMS):
            kw = {k_: inp[k_] if k_ in up else None for k_ in ("d_rgb", "d_weights", "d_depth")}
            wb = True if len(up) == 3 else fl["white_bkg"]
            args = (inp["rgbo"], inp["z"], _dirs(inp, fl), fl["mul_norm"], wb, act, shift, (NEAR, FAR))
            want, tol = R.composite_backward_ref(*args, **kw)
            for how, fn in (("autograd", R.composite_backward_autograd), ("formula", R.composite_backward_formula)):
                got = fn(*args, **kw, dt=F32)
                assert _note("composite_backward dsigma", R.worst(got[..., 3], want[..., 3], tol[..., 3])) <= 1.0, (S, act, shift, up, how, fl)
                assert _note("composite_backward dc", R.worst(got[..., :3], want[..., :3], tol[..., :3])) <= 1.0, (S, act, shift, up, how, fl)
        if shift == 0.0:
            for dirs in (None, inp["dirs"]):
                want, tol = R.sigma_to_weights_backward_ref(inp["sigma"], inp["z"], dirs, act, inp["d_weights"])
                got = R.composite_backward_formula(R.as_rgbo(inp["sigma"]), inp["z"], dirs, dirs is not None, False, act, 0.0, None, None, inp["d_weights"], None,
                                                   dt=F32)[..., 3]
                assert _note("sigma_to_weights_backward", R.worst(got, want, tol)) <= 1.0, (S, act, dirs is None)


BOUNDS_SHAPES = [(C, K) for C in (1, 63, 64, 65, 129) for K in (2, 65, 130)]


@pytest.mark.parametrize("kind", ["sorted", "unsorted", "constant"])
def test_fp32_emulation_of_get_bounds_stays_inside_the_bounds(kind):
    for C, K in BOUNDS_SHAPES:
        w, below, g = R.bounds_inputs(N, C, K, kind)
        assert int(below.min()) == 0 and int(below.max()) == C - 1            # the legal range 0 ... C - 1, both ends present: sat[C] is read
        want, tol = R.get_bounds_ref(w, below)
        assert _note("get_bounds", R.worst(R.bounds_expr(w, below), want, tol)) <= 1.0, (C, K)
        want, tol = R.get_bounds_backward_ref(below, g, C)
        assert _note("get_bounds_backward", R.worst(R.get_bounds_backward_emulation(below, g, C), want, tol)) <= 1.0, (C, K)


def _blur_inputs(S, seed=0, integer_g=False):
    gen = torch.Generator().manual_seed(S + seed)
    w = torch.rand(N, S, generator=gen)
    if S >= 2:
        w[:, S // 2] = w[:, S // 2 - 1]                                         # a tie in every row
        w[1] = 0.25                                                             # a row of ties
    g = torch.randint(-8, 9, (N, S), generator=gen).float() if integer_g else torch.randn(N, S, generator=gen)
    return w, g


@pytest.mark.parametrize("S", [1, 2, 3, 64, 65, 257])
def test_fp32_emulation_of_max_blur(S):
    w, g = _blur_inputs(S)
    assert R.violations(R.max_blur_ref(w, 0.01), O.max_blur(w, 0.01)) == 0
    assert max_abs(R.max_blur_ref(w, 0.01), TS.max_blur_expr(w.double(), 0.01)) <= 2e-7
    want, tol = R.max_blur_backward_ref(w, g)
    assert _note("max_blur_backward", R.worst(R.max_blur_backward(w, g, dt=F32), want, tol)) <= 1.0
    w, g = _blur_inputs(S, integer_g=True)                                      # every sum exact: tolerance 0
    assert R.violations(R.max_blur_backward(w, g, dt=F32), R.max_blur_backward(w, g).float()) == 0


DOT_MS = (1, 255, 256, 257, 70001)


@pytest.mark.parametrize("mode", [0, 1])
def test_fp32_emulation_of_the_dot_losses(mode):
    for M in DOT_MS:
        w, a, b = R.dot_loss_inputs(M, M + mode)
        x = R.dot3(a, b)
        assert {0.0, 1.0, -1.0} <= set(x[:min(M, 7)].tolist()) or M < 3
        scale = 1.0 if mode == 0 else 1.0 / M
        want, tol = R.dot_loss_ref(w, a, b, mode, scale)
        assert _note("weighted_dot_loss", R.worst(R.dot_loss(w, a, b, mode, scale), want, tol)) <= 1.0, M
        g = torch.tensor(0.7)
        want, tol = R.dot_loss_backward_ref(g, w, a, b, mode, scale)
        got = R.dot_loss_backward(g, w, a, b, mode, scale, dt=F32)
        for name, g_, w_, t_ in zip("wab", got, want, tol):
            assert _note("weighted_dot_loss_backward", R.worst(g_, w_, t_)) <= 1.0, (M, name)
        w, a, b = R.dot_loss_inputs(M, M + mode, dyadic=True)                   # every product exact: tolerance 0
        got, want = R.dot_loss_backward(torch.tensor(0.5), w, a, b, mode, 0.25, dt=F32), R.dot_loss_backward(torch.tensor(0.5), w, a, b, mode, 0.25)
        assert sum(R.violations(g_, w_.float()) for g_, w_ in zip(got, want)) == 0


# ------------------------------------------------------------------------------------------------ the bounds bite
S_MUT = 65


def _bwd(mut, act=R.ACT_RELU, shift=0.0, up=("d_rgb", "d_weights", "d_depth"), white=True, how="formula", S=S_MUT, inp=None):
    inp = inp or R.ray_inputs(N, S, act, shift)
    kw = {k: inp[k] if k in up else None for k in ("d_rgb", "d_weights", "d_depth")}
    args = (inp["rgbo"], inp["z"], inp["dirs"], True, white, act, shift, (NEAR, FAR))
    want, tol = R.composite_backward_ref(*args, **kw)
    fn = R.composite_backward_formula if how == "formula" else R.composite_backward_autograd
    return fn(*args, **kw, dt=F32, mut=mut)[..., 3], want[..., 3], tol[..., 3]


def _fwd(mut, name="w", act=R.ACT_RELU):
    inp = R.ray_inputs(N, S_MUT, act)
    ref = R.composite_ref(inp["rgbo"], inp["z"], inp["dirs"], True, True, act, 0.0, (NEAR, FAR))
    return R.evaluate(inp["rgbo"], inp["z"], inp["dirs"], True, True, act, 0.0, (NEAR, FAR), mut=mut)[name], ref[name][0], ref[name][1]


def _bounds_mut(mut):
    w, below, g = R.bounds_inputs(N, 65, 65, "sorted")
    below = below.clamp_max(63)                                                 # (the mutated expression itself must stay in range)
    return R.bounds_expr(w, below, mut), *R.get_bounds_ref(w, below)


def _bounds_bwd_mut(mut):
    w, below, g = R.bounds_inputs(N, 65, 65, "unsorted")
    return R.get_bounds_backward_emulation(below, g, 65, mut), *R.get_bounds_backward_ref(below, g, 65)


def _blur_mut(mut):
    w, g = _blur_inputs(65)
    return R.max_blur_backward(w, g, dt=F32, mut=mut), *R.max_blur_backward_ref(w, g)


def _dot_mut(mut, mode, which):
    w, a, b = R.dot_loss_inputs(257, 1)
    want, tol = R.dot_loss_backward_ref(torch.tensor(0.7), w, a, b, mode, 0.5)
    return R.dot_loss_backward(torch.tensor(0.7), w, a, b, mode, 0.5, dt=F32, mut=mut)[which], want[which], tol[which]


MUTATIONS = {
    "transmittance product inclusive instead of exclusive": lambda m: _fwd(("inclusive_product",) if m else ()),
    "1e-10 dropped from q": lambda m: _fwd(("no_floor",) if m else ()),
    "delta_last = 1e10 replaced by the previous delta": lambda m: _fwd(("delta_last_is_previous",) if m else ()),
    "suffix sum off by one (i >= j instead of i > j)": lambda m: _bwd(("suffix_inclusive",) if m else ()),
    "act' of softplus taken at sigma instead of sigma + shift": lambda m: _bwd(("act_grad_unshifted",) if m else (), R.ACT_SOFTPLUS, 0.5),
    "the white-background term dropped from G": lambda m: _bwd(("no_white_in_G",) if m else (), up=("d_rgb",)),
    "d_depth not divided by (far - near)": lambda m: _bwd(("depth_not_divided",) if m else (), up=("d_depth",)),
    "|d| scaling applied to delta but not to the depth term (forward)": lambda m: _fwd(("depth_term_unscaled",) if m else (), "depth"),
    "|d| scaling applied to delta but not to the depth term (backward)": lambda m: _bwd(("depth_term_unscaled",) if m else (), up=("d_depth",), how="autograd"),
    "getBounds en without the + 1": lambda m: _bounds_mut(("end_without_plus_one",) if m else ()),
    "getBounds backward en without the + 1": lambda m: _bounds_bwd_mut(("end_without_plus_one",) if m else ()),
    "the max-blur tie sent whole to one side": lambda m: _blur_mut(("tie_to_one_side",) if m else ()),
    "the back-face loss using x >= 0 instead of x > 0": lambda m: _dot_mut(("backface_ge",) if m else (), 1, 1),
    "the sign of the normal-loss gradient": lambda m: _dot_mut(("normal_sign",) if m else (), 0, 2),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_every_mutation_is_reported(name):
    got, want, tol = MUTATIONS[name](False)
    clean = R.worst(got, want, tol)
    got, want, tol = MUTATIONS[name](True)
    planted = R.worst(got, want, tol)
    print("MUTATION %-70s clean %.3f  planted %.3e" % (name, clean, planted))
    assert clean <= 1.0 < planted


def test_comparator_reports_nan_inf_and_zero_tolerance():
    want, tol = torch.ones(4, dtype=F64), torch.full((4,), 1e-3, dtype=F64)
    assert R.worst(torch.tensor([1.0, 1.0005, 1.0, 1.0]), want, tol) == pytest.approx(0.5, rel=1e-3)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert R.worst(torch.tensor([1.0, bad, 1.0, 1.0]), want, tol) == float("inf")
    assert R.worst(torch.ones(4), want, torch.zeros(4)) == 0.0
    assert R.worst(torch.tensor([1.0, 1.0, 1.0, 1.0 + 2.0 ** -20]), want, torch.zeros(4)) == float("inf")
    assert R.worst(torch.ones(4), want, torch.tensor([1.0, float("inf"), 1.0, 1.0])) == float("inf")
    assert R.worst(torch.zeros(0), torch.zeros(0), torch.zeros(0)) == 0.0
    assert R.violations(torch.tensor([0.0, 1.0]), torch.tensor([-0.0, 1.0])) == 0
    assert R.violations(torch.tensor([float("nan"), 1.0]), torch.tensor([float("nan"), 1.0])) == 1


def test_the_old_gate_lets_a_wrong_backward_through():
    """The motivation, kept as a regression.  Inputs of test_gpu_parity.test_weights_and_composite_backward_vs_autograd at S = 1024 with softplus
    and sigma_shift = 0.5, the upstream gradient that of a mean-squared-error loss over the batch, d_rgb = 2 (rgb - target) / (3 N), as in
    training.  A backward that takes softplus' at sigma instead of sigma + shift is wrong by more than 10 % on most elements; it passes that
    test's gate, 2e-5 * max(1, max |want|), and fails the comparator."""
    S, act, shift = 1024, R.ACT_SOFTPLUS, 0.5
    gen = torch.Generator().manual_seed(S)
    z = torch.sort(torch.rand(N, S, generator=gen) * 4 + 2, dim=-1)[0]
    rgbo = torch.cat((torch.rand(N, S, 3, generator=gen), torch.randn(N, S, 1, generator=gen) * 2), -1)
    dirs = torch.randn(N, 3, generator=gen) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
    rgb = R.evaluate(rgbo, z, dirs, True, True, act, shift)["rgb"]
    d_rgb = 2.0 * (rgb - torch.rand(N, 3, generator=gen)) / (3 * N)
    args = (rgbo, z, dirs, True, True, act, shift, None, d_rgb, None, None)
    want, tol = R.composite_backward_ref(*args)
    want, tol = want[..., 3], tol[..., 3]
    clean = R.composite_backward_formula(*args, dt=F32)[..., 3]
    wrong = R.composite_backward_formula(*args, dt=F32, mut=("act_grad_unshifted",))[..., 3]
    old_gate = 2e-5 * max(1.0, float(want.abs().max()))
    off = float(((wrong - want).abs() > 0.1 * want.abs()).double().mean())
    print("old gate %.3e: clean %.3e wrong %.3e; comparator: clean %.3f wrong %.3e; elements off by more than 10 %%: %.0f %%" % (
        old_gate, max_abs(clean, want), max_abs(wrong, want), R.worst(clean, want, tol), R.worst(wrong, want, tol), 100.0 * off))
    assert max_abs(clean, want) <= old_gate and R.worst(clean, want, tol) <= 1.0
    assert off >= 0.5
    assert max_abs(wrong, want) <= old_gate
    assert R.worst(wrong, want, tol) > 1.0
