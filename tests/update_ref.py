"""The fp64 yardstick of the last stretch of a training iteration: gradients in, new parameters out.  adam_kernel / bwd_launch_adam
(nerf_amd/csrc/bwd_kernels.hip, ops.adam_step, nerf_amd.optim.Adam) and the global-norm clip of TrainStep(grad_clip=...)
(nerf_amd/training.py).  tests/test_gpu_update.py compares the kernel and the training step with it; tests/test_update_ref_host.py tests
the yardstick itself on the CPU.  The library is built with -ffp-contract=off and without any fast-math switch: every fp32 operation
below is one rounding.

SPECIFICATION (torch.optim.Adam's single-tensor rule without weight decay / amsgrad, in fp64 on the fp32 inputs), g' = g grad_scale:

    m' = m + w1 (g' - m)          v' = b2 v + w2 g'^2          denom = sqrt(v') / bc2_sqrt + epsf          p' = p - step_size m' / denom

The scalars are the fp32 values the kernel forms (kernel_scalars): with t = the counter AFTER its increment and Python doubles as torch
computes them, step_size = fp32(lr / (1 - beta1^t)), bc2_sqrt = fp32(sqrt(1 - beta2^t)), w1 = fp32(1 - beta1), w2 = fp32(1 - beta2),
b2 = fp32(beta2), epsf = fp32(eps), grad_scale = fp32(grad_scale), all promoted to fp64: the only admitted error is the per-element
rounding of the kernel's operation list

    g1 = fl(g gs)     d = fl(g1 - m)   e = fl(w1 d)   m' = fl(m + e)     a = fl(v b2)   q = fl(g1 g1)   c = fl(w2 q)   v' = fl(a + c)
    s = sqrtf(v')     r = fl(s / bc2_sqrt)   denom = fl(r + epsf)       h = fl(m' / denom)   k = fl(step_size h)   p' = fl(p - k)

BOUNDS (adam_ref).  u = 2^-24; one rounding is |fl(x) - x| <= u |x| + ETA / 2 with ETA = 2^-149 the smallest subnormal (fp32 denormals
are kept on gfx950; a sum or difference that lands in the subnormal range is exact, so only products and quotients carry ETA / 2).
Division is charged DIV_C u = 5 u and sqrtf SQRT_C u = 6 u, the device library's documented 2.5 and 3 ulp, as everywhere in this suite
(ref_forward_ref) -- the bound does not lean on the compiler's correctly-rounded default.  Every e(.) below is a bound on |device value -
fp64 value|; the products of bounds are kept (no first-order truncation), so nothing is dropped.  (dp, dm, dv) are bounds on the
errors the INPUT state already carries (0 for one step from given fp32 state; the previous step's bounds in a trajectory).

    g1      e(g) = u |g'| + ETA/2   (0 when grad_scale == 1: the product is exact)
    v'      e(q) = 2 |g'| e(g) + e(g)^2 + u (|g'| + e(g))^2 + ETA/2          e(c) = w2 e(q) + u w2 (g'^2 + e(q)) + ETA/2
            e(a) = b2 dv + u b2 (v + dv) + ETA/2                             e(v) = e(a) + e(c) + u (v' + e(a) + e(c))
            -> to first order 5 u v' + 2 ETA with exact inputs: b2 v carries 2 u, w2 g'^2 carries 5 u with a scale and 3 u without
    m'      the exact map is m' = (1 - w1) m + w1 g': an input error dm arrives as |1 - w1| dm (not as the (1 + w1) dm an interval walk
            through d and e would give); the roundings are those of d, e and the final sum:
            r(d) = u (|g' - m| + e(g) + dm)      r(e) = u w1 (|g' - m| + e(g) + dm + r(d)) + ETA/2
            e(m) = |1 - w1| dm + w1 (e(g) + r(d)) + r(e) + u (|m'| + all of the former)
            -> u (w1 |g'| + 2 w1 |g' - m| + |m'|) with exact inputs
    denom   |sqrt(x) - sqrt(v')| <= min(|x - v'| / sqrt(v'), sqrt(|x - v'|)) =: ds   (the second form holds at v' = 0, where the first
            says nothing);  e(s) = ds + SQRT_C u (sqrt(v') + ds);  e(r) = e(s) / bc + DIV_C u (sqrt(v') + e(s)) / bc + ETA/2;
            e(denom) = e(r) + u (denom + e(r)).   denom >= epsf > 0 and e(denom) < denom (asserted), lo = denom - e(denom)
    p'      e(h) = e(m) / lo + |m'| e(denom) / (denom lo) + DIV_C u (|m'| + e(m)) / lo + ETA/2
            e(k) = step_size e(h) + u step_size (|m'| / denom + e(h)) + ETA/2
            e(p) = dp + e(k) + u (|p'| + dp + e(k))
            -> the final rounding u |p'| is attained (a p' just above a power of two rounded by half an ulp), so the gate on p' is sharp

CLIPPING (clip_gates).  The specification is torch's: k = min(c / (n + 1e-6), 1) with n the 2-norm of ALL gradients of the
fine and the proposal network together (train.py:117-121, 217), every gradient multiplied by the one fp32 scalar k.  The flat path
evaluates it as one vector_norm and one mul_ over the FlatGradients buffer, the per-tensor path as clip_grad_norm_.  Both are library
reductions whose order of additions is not ours, so the limit on k against the fp64 value c / (n64 + 1e-6) is not chosen here: it is the
relative error of torch's own fp32 norm on the very snapshot, measured against n64, plus 3 u for the add, the reciprocal-multiply
(`float / tensor` is tensor.reciprocal() * float in torch) and the rounding of k.  STRUCTURE is exact: clipped == fl(unclipped * k) bit
for bit for that one k over every element of every tensor, which rules out a range that escaped the scale or entered the norm stale.
From fresh state exp_avg == fl(w1 * clipped) bit for bit (d = g - 0 and 0 + e are exact) and exp_avg_sq obeys e(v) with v = 0."""
import math

import numpy as np
import torch

from ray_stages_ref import violations, worst              # noqa: F401  (one comparator for the whole suite)
from ref_forward_ref import DIV_C, SQRT_C, U

F32, F64 = torch.float32, torch.float64
ETA = 2.0 ** -149
HALF_ETA = 0.5 * ETA
ADAM_MAX = 48                                              # bwd_kernels.hip: tensors per table launch
GRID_PASS = 32 * 256                                       # one pass of the kernel's 32 x 256 grid


def f32c(x):
    """a Python double as the fp32 value the kernel forms from it, widened back"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the scalars
SCALARS = ((0, 3e-4, 0.9, 0.999, 1e-8), (9, 1e-3, 0.9, 0.999, 1e-8), (6199, 4.5e-6, 0.9, 0.999, 1e-8), (999, 1e-2, 0.5, 0.9, 1e-6))   # (t0, lr, beta1, beta2, eps)
GRAD_SCALES = (1.0, 0.5, 1.0 / 3.0)
COUNTS = (1, 47, 48, 49, 97)                               # one, one, one, two and three table launches
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193, 3 * 8192 + 5)
REGIMES = ("generic", "fresh", "g=0", "tiny", "cancelling")
T_END = 2 ** 24                                            # the fp32 counter counts exactly up to here


def kernel_scalars(t, lr, beta1, beta2, eps, grad_scale=1.0):
    """t = the counter AFTER the increment -> the fp32 scalars of adam_kernel as Python floats (Python doubles first, as torch forms them)"""
    t = float(t)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    return {"step_size": f32c(lr / bc1) if bc1 != 0.0 else float("inf"), "bc2_sqrt": f32c(math.sqrt(bc2)), "w1": f32c(1.0 - beta1), "w2": f32c(1.0 - beta2),
            "b2": f32c(beta2), "eps": f32c(eps), "gs": f32c(grad_scale)}


# ------------------------------------------------------------------------------------------------ one Adam step: fp64 specification, bounds
def adam_eval(p, g, m, v, sc, dt=F64, mut=()):
    """The operation list in dtype dt on tensors of any shape: fp64 = the specification, fp32 = the emulation of the kernel's element
    loop (every torch operation rounds once, like the uncontracted kernel), with the planted element-level faults `mut` -> (p', m', v')."""
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    g1 = g * sc["gs"]
    w1 = sc["w1"] if "lerp_beta1" not in mut else 1.0 - sc["w1"]          # (exact in fp64 for 0.9 / 0.5; a fault anyway)
    m2 = m + w1 * (g1 - m)
    gq = g if "scale_not_squared" in mut else g1
    v2 = v * sc["b2"] + sc["w2"] * (gq * gq)
    if "eps_in_sqrt" in mut:
        denom = torch.sqrt(v2 + sc["eps"]) / sc["bc2_sqrt"]
    elif "eps_before_division" in mut:
        denom = (torch.sqrt(v2) + sc["eps"]) / sc["bc2_sqrt"]
    else:
        denom = torch.sqrt(v2) / sc["bc2_sqrt"] + sc["eps"]
    p2 = p - sc["step_size"] * ((m if "old_m" in mut else m2) / denom)
    return p2, m2, v2


def adam_ref(p, g, m, v, sc, dp=0.0, dm=0.0, dv=0.0):
    """-> {"p": (want, tol), "m": ..., "v": ...} in fp64: the specification and the bounds of the module docstring"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p2, m2, v2 = adam_eval(p, g, m, v, sc, F64)
    w1, w2, b2, bc, step = sc["w1"], sc["w2"], sc["b2"], sc["bc2_sqrt"], sc["step_size"]
    g1 = g * sc["gs"]
    eg = torch.zeros_like(g1) if sc["gs"] == 1.0 else U * g1.abs() + HALF_ETA
    # v'
    eq = 2.0 * g1.abs() * eg + eg * eg + U * (g1.abs() + eg) ** 2 + HALF_ETA
    ec = w2 * eq + U * w2 * (g1 * g1 + eq) + HALF_ETA
    ea = b2 * dv + U * b2 * (v + dv) + HALF_ETA
    ev = ea + ec + U * (v2 + ea + ec)
    # m'
    diff = (g1 - m).abs()
    rd = U * (diff + eg + dm)
    re = U * w1 * (diff + eg + dm + rd) + HALF_ETA
    em = abs(1.0 - w1) * dm + w1 * (eg + rd) + re
    em = em + U * (m2.abs() + em)
    # denom
    sv = torch.sqrt(v2)
    ds = torch.minimum(torch.where(sv > 0, ev / sv.clamp_min(1e-300), torch.full_like(ev, float("inf"))), torch.sqrt(ev))
    es = ds + SQRT_C * U * (sv + ds)
    er = es / bc + DIV_C * U * (sv + es) / bc + HALF_ETA
    denom = sv / bc + sc["eps"]
    eden = er + U * (denom + er)
    lo = denom - eden
    assert bool((lo > 0).all()), "the bound of denom says nothing: e(denom) >= denom"
    # p'
    eh = em / lo + m2.abs() * eden / (denom * lo) + DIV_C * U * (m2.abs() + em) / lo + HALF_ETA
    ek = step * eh + U * step * (m2.abs() / denom + eh) + HALF_ETA
    ep = dp + ek + U * (p2.abs() + dp + ek)
    return {"p": (p2, ep), "m": (m2, em), "v": (v2, ev)}


# ------------------------------------------------------------------------------------------------ the inputs both test modules use
P_GUARD, G_GUARD, M_GUARD, V_GUARD = -7.25, 11.5, 3.0625, 5.75        # the sentinels of everything outside the views


def _gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(repr(key).encode(), "little") % (2 ** 31 - 1))


class Table:
    """`count` tensors as views into one flat buffer per role (p, g, m, v; fp32, CPU): tensor i has LENGTHS[i % 11] elements and starts
    at an ODD element offset -- what FlatGradients hands the kernel whenever an odd-sized bias sits in front -- with at least one guard
    element before and after it; EVERYTHING outside the views is guard space, holds the role's sentinel and must come back bit-identical.
    Element j of tensor i is of value regime REGIMES[(i + j) % 5]: every tensor of five or more elements holds all five, its ragged tail
    included, and the one-element tensors 0, 11, 22, 33, 44 meet one each.  With 11 lengths, tensors 37..47 and 48..58 put one tensor of
    each length on either side of the 47 / 48 table seam (count 97)."""

    def __init__(self, count):
        self.count = count
        self.ranges, cur = [], 0
        for i in range(count):
            n = LENGTHS[i % len(LENGTHS)]
            cur += cur % 2                                  # the guard in front sits at an even offset: the view starts odd
            self.ranges.append((cur + 1, n))
            cur += n + 2
        self.total = cur
        assert all(o % 2 == 1 for o, _ in self.ranges)
        self.mask = torch.zeros(self.total, dtype=torch.bool)
        tensor_id = torch.zeros(self.total, dtype=torch.int64)
        within = torch.zeros(self.total, dtype=torch.int64)
        for i, (o, n) in enumerate(self.ranges):
            assert not bool(self.mask[o - 1:o + n + 1].any())
            self.mask[o:o + n] = True
            tensor_id[o:o + n] = i
            within[o:o + n] = torch.arange(n)
        assert not bool(self.mask[[o - 1 for o, _ in self.ranges]].any()) and not bool(self.mask[[o + n for o, n in self.ranges]].any())
        self.tensor_id, self.regime = tensor_id, (tensor_id + within) % len(REGIMES)
        gn = _gen("adam table", count)
        N = self.total
        rnd = lambda: torch.rand(N, generator=gn)
        sign = lambda: torch.where(rnd() < 0.5, -1.0, 1.0)
        p = torch.randn(N, generator=gn)
        p[within % 7 == 3] = 0.0                            # parameters at zero: the update term alone decides p'
        g = sign() * 10.0 ** (8.0 * rnd() - 5.0)            # eight decades, |g| <= 1e3
        m = 1e-3 * torch.randn(N, generator=gn)
        v = 1e-5 * rnd()
        r = self.regime
        m[r == 1], v[r == 1] = 0.0, 0.0                     # fresh state
        g[r == 2] = 0.0                                     # g = 0 with live moments
        tiny = r == 3                                       # g, m down to 1e-24, v down to 1e-40 (subnormal): g'^2 underflows, eps decides
        g[tiny] = (sign() * 10.0 ** (-24.0 + 4.0 * rnd()))[tiny]
        m[tiny] = (sign() * 10.0 ** (-24.0 + 4.0 * rnd()))[tiny]
        v[tiny] = (10.0 ** (-40.0 + 3.0 * rnd()))[tiny]
        can = r == 4                                        # g = m (1 + 1e-6 xi), v = m^2
        g[can] = (m * (1.0 + 1e-6 * torch.randn(N, generator=gn)))[can]
        v[can] = (m * m)[can]
        assert float(g.abs().max()) <= 1e3 and bool((v >= 0).all())
        for t, s in ((p, P_GUARD), (g, G_GUARD), (m, M_GUARD), (v, V_GUARD)):
            t[~self.mask] = s
        self.p, self.g, self.m, self.v = p, g, m, v

    def views(self, flat):
        return [flat[o:o + n] for o, n in self.ranges]


_TABLES = {}


def table(count):
    """the inputs of one tensor count, built once and never written (every run clones)"""
    if count not in _TABLES:
        _TABLES[count] = Table(count)
    return _TABLES[count]


# ------------------------------------------------------------------------------------------------ the launcher, emulated
ELEMENT_FAULTS = ("eps_before_division", "eps_in_sqrt", "scale_not_squared", "lerp_beta1", "old_m")
ADAM_FAULTS = ("bias_correction_at_t0",) + ELEMENT_FAULTS + ("tensor_48_skipped", "tensor_47_twice", "tail_untouched", "counter_per_launch")


class Emulation:
    """bwd_launch_adam + adam_kernel in torch fp32 on the CPU: the counter incremented once, the tensor list cut into tables of ADAM_MAX,
    every element through adam_eval in fp32; with planted faults `mut`.  tests/test_gpu_update.py has the same interface over ops.adam_step."""

    def __init__(self, mut=()):
        self.mut = tuple(mut)

    def adam(self, tab, state, t0, lr, beta1, beta2, eps, grad_scale, lr_dev=None, g=None):
        """state = (p, m, v) flat fp32 buffers (not written) -> (p', m', v', g after the call, the counter after the call).
        lr_dev: the value of the device scalar that overrides the argument `lr` (None: none is passed)"""
        mut = self.mut
        lr = lr if lr_dev is None else lr_dev
        p, m, v = (x.clone() for x in state)
        g = (tab.g if g is None else g).clone()
        counter = np.float32(t0) + np.float32(1.0)
        launches = range(0, tab.count, ADAM_MAX)
        if "counter_per_launch" in mut:
            counter = np.float32(t0)
        for base in launches:
            if "counter_per_launch" in mut:
                counter = counter + np.float32(1.0)
            t = float(counter) - (1.0 if "bias_correction_at_t0" in mut else 0.0)
            sc = kernel_scalars(t, lr, beta1, beta2, eps, grad_scale)
            ids = list(range(base, min(base + ADAM_MAX, tab.count)))
            if "tensor_48_skipped" in mut:
                ids = [i for i in ids if i != 48]
            if "tensor_47_twice" in mut and 47 in ids:
                ids.append(47)
            for i in ids:
                o, n = tab.ranges[i]
                if "tail_untouched" in mut:
                    n -= n % 256
                s = slice(o, o + n)
                p[s], m[s], v[s] = adam_eval(p[s], g[s], m[s], v[s], sc, F32, mut)
        return p, m, v, g, float(counter)


# ------------------------------------------------------------------------------------------------ the kernel checks, shared by the host and the GPU module
def _adam_gates(tag, tab, state, out, t0, scal, gs):
    """one call against the specification: every element of every view under its bound, everything outside the views and the whole of g
    bit-identical, the counter t0 + 1 exactly -> [(name, value, limit)]"""
    p, m, v, g, counter = out
    _, lr, b1, b2, eps = scal
    ref = adam_ref(state[0], tab.g, state[1], state[2], kernel_scalars(t0 + 1, lr, b1, b2, eps, gs))
    items, msk = [], tab.mask
    for k, got in (("p", p), ("m", m), ("v", v)):
        want, tol = ref[k]
        items.append(("update adam %s %s'" % (tag, k), worst(got[msk], want[msk], tol[msk]), 1.0))
    guards = sum(violations(a[~msk], b[~msk]) for a, b in ((p, state[0]), (m, state[1]), (v, state[2])))
    items.append(("update adam %s guard elements changed" % tag, guards, 0))
    items.append(("update adam %s gradient elements changed" % tag, violations(g, tab.g), 0))
    items.append(("update adam %s |counter - (t0 + 1)|" % tag, abs(counter - (t0 + 1)), 0))
    return items


def _bits_differ(a, b):
    return sum(int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(a[:3], b[:3])) + (0 if a[4] == b[4] else 1)


def kernel_case_gates(impl, count, si, gs):
    """One (tensor count, scalar set, grad_scale): the call with lr as an argument against the specification; the call with lr through
    lr_dev (and a WRONG lr argument, which the kernel must not read) bit for bit equal to it; at grad_scale 0.5 the call with g / 2 and
    scale 1 bit for bit equal as well (a power of two commutes with every rounding short of the subnormal range; no g here is that small
    once halved: the smallest is 1e-24)."""
    tab = table(count)
    scal = SCALARS[si]
    t0, lr, b1, b2, eps = scal
    state = (tab.p, tab.m, tab.v)
    tag = "tensors=%d t0=%d lr=%g b=(%g,%g) eps=%g gs=%.3g" % (count, t0, lr, b1, b2, eps, gs)
    out = impl.adam(tab, state, t0, lr, b1, b2, eps, gs)
    items = _adam_gates(tag, tab, state, out, t0, scal, gs)
    dev = impl.adam(tab, state, t0, lr * 7.0, b1, b2, eps, gs, lr_dev=lr)
    items.append(("update adam %s lr_dev: bits that differ from the lr-argument call" % tag, _bits_differ(out, dev), 0))
    if gs == 0.5:
        g_half = torch.where(tab.mask, tab.g * 0.5, tab.g)
        half = impl.adam(tab, state, t0, lr, b1, b2, eps, 1.0, g=g_half)
        items.append(("update adam %s bits that differ from g / 2 with scale 1" % tag, _bits_differ(out, half), 0))
    return items


def kernel_cases():
    """every (count, scalar set) with the grad_scale rotating, and every grad_scale for every scalar set at 49 tensors (across the seam)"""
    cases = [(c, si, GRAD_SCALES[(ci + si) % 3]) for ci, c in enumerate(COUNTS) for si in range(len(SCALARS))]
    cases += [(49, si, gs) for si in range(len(SCALARS)) for gs in GRAD_SCALES if (49, si, gs) not in cases]
    return tuple(cases)


def counter_end_gates(impl):
    """from t0 = 2^24 - 2 two calls leave 2^24 - 1 and 2^24 exactly (the documented limit of the fp32 counter; nothing beyond it is
    tested), each call's outputs within the bound of one step from the state it was given"""
    tab = table(49)
    _, lr, b1, b2, eps = SCALARS[1]
    state, items = (tab.p, tab.m, tab.v), []
    for t0 in (T_END - 2, T_END - 1):
        out = impl.adam(tab, state, t0, lr, b1, b2, eps, 1.0)
        items += _adam_gates("tensors=49 t0=2^24%+d" % (t0 - T_END), tab, state, out, t0, (t0, lr, b1, b2, eps), 1.0)
        state = out[:3]
    return items


# ------------------------------------------------------------------------------------------------ the optimizer class: a three-step trajectory
CLASS_SHAPES = ((256, 63), (256,), (3, 8193), (1,), (65, 129), (257,))
CLASS_STEPS, CLASS_GS, CLASS_LR = 3, 1.0 / 3.0, 1e-3


def class_inputs():
    """-> (parameters, [gradients of step 1, 2, 3]) fp32 CPU, six tensors of mixed length, gradients over eight decades"""
    gn = _gen("adam class")
    params = [torch.randn(s, generator=gn) for s in CLASS_SHAPES]
    grads = [[torch.where(torch.rand(s, generator=gn) < 0.5, -1.0, 1.0) * 10.0 ** (8.0 * torch.rand(s, generator=gn) - 5.0) for s in CLASS_SHAPES]
             for _ in range(CLASS_STEPS)]
    return params, grads


def class_reference(params, grads, betas=(0.9, 0.999), eps=1e-8):
    """The reference trajectory: the fp64 specification iterated on its OWN fp64 state from m = v = 0 (never on the code under test's),
    the bound propagated step by step (adam_ref's dp, dm, dv) -> per tensor {"p": (want, tol), "m": ..., "v": ...} after CLASS_STEPS"""
    out = []
    for i, p0 in enumerate(params):
        st = {"p": (p0.double(), 0.0), "m": (torch.zeros_like(p0, dtype=F64), 0.0), "v": (torch.zeros_like(p0, dtype=F64), 0.0)}
        for t in range(1, CLASS_STEPS + 1):
            sc = kernel_scalars(t, CLASS_LR, betas[0], betas[1], eps, CLASS_GS)
            st = adam_ref(st["p"][0], grads[t - 1][i], st["m"][0], st["v"][0], sc, dp=st["p"][1], dm=st["m"][1], dv=st["v"][1])
        out.append(st)
    return out


def class_gates(got, ref):
    """got: per tensor (p, exp_avg, exp_avg_sq) after the three steps"""
    items = []
    for k, j in (("p", 0), ("m", 1), ("v", 2)):
        items.append(("update Adam(grad_scale=1/3) three steps from fresh state %s'" % k, max(worst(g[j], *r[k]) for g, r in zip(got, ref)), 1.0))
    return items


def emulate_class(params, grads, mut=()):
    """the class on the CPU: three launches of the emulation over the six tensors (one table)"""
    p, m, v = [x.clone() for x in params], [torch.zeros_like(x) for x in params], [torch.zeros_like(x) for x in params]
    for t in range(1, CLASS_STEPS + 1):
        sc = kernel_scalars(t, CLASS_LR, 0.9, 0.999, 1e-8, CLASS_GS)
        for i in range(len(p)):
            p[i], m[i], v[i] = adam_eval(p[i], grads[t - 1][i], m[i], v[i], sc, F32, mut)
    return list(zip(p, m, v))


# ------------------------------------------------------------------------------------------------ global-norm clipping
def flat_of(tensors, dt=None):
    return torch.cat([t.detach().reshape(-1) if dt is None else t.detach().reshape(-1).to(dt) for t in tensors])


def norm64(tensors):
    """the 2-norm of all tensors together in fp64 (the sum of squares in fp64 over a few 1e5 elements: relative error ~1e-14)"""
    return float(torch.linalg.vector_norm(flat_of(tensors, F64)))


def flat_coefficient(unclipped, c):
    """training.py's own expression on the snapshot, on the snapshot's device (the same library reduction over the same flat order)"""
    return torch.clamp(c / (torch.linalg.vector_norm(flat_of(unclipped)) + 1e-6), max=1.0)


def per_tensor_coefficient(unclipped, c):
    """clip_grad_norm_ on a clone of the snapshot -> (k, the clipped clones, torch's fp32 total norm)"""
    ps = [torch.nn.Parameter(torch.zeros_like(t)) for t in unclipped]
    for p, t in zip(ps, unclipped):
        p.grad = t.detach().clone()
    total = torch.nn.utils.clip_grad_norm_(ps, c)
    return torch.clamp(c / (total + 1e-6), max=1.0), [p.grad for p in ps], total


def clip_gates(tag, unclipped, clipped, c, flat, exp_avg=None, exp_avg_sq=None, betas=(0.9, 0.999), twin=None):
    """Checks 1-5 of an ACTIVE clip on the two snapshots of one step (lists of fp32 tensors in the optimizer's parameter order, any
    device): structure, the coefficient against fp64, the norm a user relies on, the moments the optimizer formed from fresh state, and
    the unclipped gradients against the twin's -> [(name, value, limit)]"""
    items = []
    n64 = norm64(unclipped)
    if flat:
        k = flat_coefficient(unclipped, c)
        n32 = float(torch.linalg.vector_norm(flat_of(unclipped)))
    else:
        k, clones, total = per_tensor_coefficient(unclipped, c)
        n32 = float(total)
        items.append((tag + " clipped != clip_grad_norm_ on a clone of the snapshot (elements)", sum(violations(a, b) for a, b in zip(clipped, clones)), 0))
    assert k.dtype == F32 and k.numel() == 1
    # 1. structure: one fp32 scalar over every element
    items.append((tag + " clipped != fl(unclipped * k) (elements)", sum(violations(a, b * k) for a, b in zip(clipped, unclipped)), 0))
    # 2. the coefficient: the limit is the measured error of torch's fp32 norm on this snapshot + 3 u
    norm_err = abs(n32 - n64) / n64
    limit = norm_err + 3.0 * U
    items.append((tag + " torch's fp32 norm of the snapshot vs fp64 (rel; recorded, it sets the next limit)", norm_err, norm_err))
    k64 = min(c / (n64 + 1e-6), 1.0)
    items.append((tag + " k vs c / (n64 + 1e-6) (rel)", abs(float(k) - k64) / k64, limit))
    # 3. what a user relies on: the norm of what the optimizer reads is at most c (1 + limit + u); written as the excess over c
    items.append((tag + " fp64 norm of the clipped gradients / c - 1", norm64(clipped) / c - 1.0, limit + U))
    # 4. the optimizer saw the clipped gradients (fresh state, grad_scale 1)
    if exp_avg is not None:
        w1 = f32c(1.0 - betas[0])
        items.append((tag + " exp_avg != fl(w1 * clipped) (elements)", sum(violations(a, b * w1) for a, b in zip(exp_avg, clipped)), 0))
        sc = kernel_scalars(1, 1.0, betas[0], betas[1], 1e-8)              # (v' depends on w2, b2 and grad_scale alone)
        worst_v = 0.0
        for a, b in zip(exp_avg_sq, clipped):
            z = torch.zeros_like(b, device="cpu")
            worst_v = max(worst_v, worst(a, *adam_ref(z, b.cpu(), z, z, sc)["v"]))
        items.append((tag + " exp_avg_sq vs (1 - beta2) clipped^2", worst_v, 1.0))
    # 5. clipping changes nothing upstream of itself
    if twin is not None:
        items.append((tag + " unclipped != the unclipped twin's gradients (elements)", sum(violations(a, b) for a, b in zip(unclipped, twin)), 0))
    return items


CLIP_FAULTS = ("range_escaped_scale", "stale_range_in_norm", "scale_not_clamped", "norm_of_first_tensor_only")


def emulate_clip(unclipped, c, flat, mut=()):
    """the two implementations on the CPU, with planted faults -> the clipped gradients"""
    g = [t.clone() for t in unclipped]
    if flat:
        buf = flat_of(g)
        if "stale_range_in_norm" in mut:                    # the last tensor's range still holds another window's values when the norm is taken
            stale = buf.clone()
            stale[-g[-1].numel():] = 3.0 * stale[-g[-1].numel():] + 1.0
            nrm = torch.linalg.vector_norm(stale)
        elif "norm_of_first_tensor_only" in mut:
            nrm = torch.linalg.vector_norm(buf[:g[0].numel()])
        else:
            nrm = torch.linalg.vector_norm(buf)
        k = c / (nrm + 1e-6)
        if "scale_not_clamped" not in mut:
            k = torch.clamp(k, max=1.0)
        out = [t * k for t in g]
    else:
        _, out, _ = per_tensor_coefficient(g, c)
    if "range_escaped_scale" in mut:                        # a range that was outside the buffer when the scale ran
        out[1] = g[1].clone()
    return out
