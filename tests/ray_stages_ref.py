"""The fp64 yardstick of the per-ray stages between the MLP kernels (nerf_amd/csrc/sample_kernels.hip, device_common.h wave_sigma_to_weights):
sigma -> weights, compositing, max-blur, getBounds, the weighted-dot losses and their hand-derived backwards.  tests/test_gpu_ray_stages.py
compares the kernels with it element by element; tests/test_ray_stages_ref_host.py tests the yardstick itself on the CPU.

SPECIFICATION.  The fp32 inputs are taken as given, converted to fp64, and the expressions of tests/torch_spec.py (weights_expr,
max_blur_expr, bounds_expr) plus the compositing (nerf_base.py:91-113) and the two dot losses (ref_model.py:127-143) are evaluated exactly:

    zn_s = z_s |d| (mul_norm) or z_s          delta_s = zn_{s+1} - zn_s,  delta_{S-1} = 1e10        x_s = sigma_s + shift
    m_s = exp(-act(x_s) delta_s)              q_s = m_s + 1e-10           T_s = prod_{j<s} q_j      w_s = (1 - m_s) T_s
    rgb = sum_s w_s c_s [+ 1 - sum_s w_s]     depth = (sum_s w_s zn_s - near) / (far - near)        normal_img = (sum_s w_s <n_s, cam> + 1) / 2

Gradients are torch.autograd's, in fp64.  `evaluate(..., dt=torch.float32)` is the SAME code in fp32 -- the emulation the host test holds
against every bound -- with the two things the kernels do in fp64 done in fp64 there too (the transmittance product, the prefix sum of
getBounds and of the backward's G w), and the per-ray sums taken as the wave takes them (per-lane partials, then a 6-level tree).

BOUNDS.  u = 2^-24 (one fp32 rounding, relative), TINY = 2^-126 (a result the device may flush to zero); the transcendental constants are the
ones tests/ref_forward_ref.py already assumes for the device library: expf 3 ulp = 6 u, log1pf 2 ulp = 4 u, sqrtf 3 ulp = 6 u, division
2.5 ulp = 5 u.  e(v) is the bound of |computed v - exact v|; products of two bounds are kept where either factor can be large, otherwise
covered by the factor ONE = 1.01.  Every line below is one fp32 operation of the kernels.

  |d|      three products and two additions of non-negative terms: 3 u on the radicand, halved by the root, + 6 u:     E_NRM = 7.5 u
  zn       fl(z |d|^):  e(zn) = (E_NRM + u) |zn|;            without mul_norm zn = z, e = 0
  delta    both zn carry the SAME |d|^, so that error scales delta; the two roundings of the products do not cancel:
           e(delta) = (E_NRM + u) |delta| + u (|zn_s| + |zn_{s+1}|) + u |delta|;   without mul_norm one subtraction: u |delta|;   1e10 is exact
  x        e(x) = u |x| when shift != 0 (one addition), else 0
  act      relu: e(x) where x >= -e(x);  identity: e(x);
           softplus = log1p(exp(x)), x <= 20: d/dx = sigmoid <= 1 and t / ((1 + t) log1p(t)) <= 1, so e = sigmoid(x + e(x)) e(x) + (6 + 4) u softplus(x)
           (+ 2.1e-9 where the rounding of x can cross the threshold 20: |x - log1p(exp(x))| there)
  a        = act * delta:   e(a) = e(act) |delta| + |act| e(delta) + e(act) e(delta) + u |a|
  m        = expf(-a^):     e(m) = max(exp(-(a - e(a))) - m, m - exp(-(a + e(a)))) + 6 u exp(-(a - e(a))) + TINY
  alpha    = 1 - m:         e(alpha) = e(m) + u |alpha|        -- the `1 - expf` regime of near-empty rays: e(alpha) / alpha ~ u / alpha, by specification
  q        = m + 1e-10f:    e(q) = e(m) + u 1e-10 (the fp32 constant) + u q;       rho = e(q) / q
  T        product in fp64, rounded once:  e(T) = T (expm1(sum_{j<s} rho_j) + u + S 2^-52) + TINY
  w        = alpha T:       e(w) = ONE (e(alpha) T + alpha e(T) + u |w|) + e(alpha) e(T) + TINY

  per-ray sums  sum_s t_s of fp32 terms: each lane adds its ceil(S/64) terms in any order, the 64 lanes are combined by a tree or scan of
           depth 6 in any pairing; a term passes through at most D = ceil(S/64) - 1 + 6 additions:   e = sum e(t_s) + ONE D u sum (|t_s| + e(t_s))
  rgb      t = w c:  e(t) = ONE (e(w) |c| + u |w c|);  white background: W = sum w the same way, bg = 1 - W: e(bg) = e(W) + u |bg|, and one more
           addition: + u |rgb|
  depth    t = w zn: e(t) = ONE (e(w) |zn| + |w| e(zn) + u |w zn|);  minus near: + u |acc - near|;  far - near: u relative;  the quotient: 5 u
  normal   <n, cam> = (n0 c0 + n1 c1) + n2 c2:  e = ONE 3 u sum_k |n_k c_k|;  t = w <n, cam>;  + 1: u |acc + 1|;  * 0.5 exact

  backward (sample_kernels.hip weights_backward_kernel; G_j = dL/dw_j):
           dL/dm_j = -G_j T_j + S_j / q_j,  S_j = sum_{i>j} G_i w_i,     dL/dsigma_j = dL/dm_j (-delta_j m_j) act'(x_j),     dL/dc_jk = w_j d_rgb_k
  G        = d_w + ((dr c0 + dg c1) + db c2) - bg + dd zn,  bg = (dr + dg) + db,  dd = d_depth / (far - near):
           e(G) = ONE (3 u sum_k |d_k c_k| + 2 u BG + 7 u |dd zn| + |dd| e(zn) + 4 u (|d_w| + sum_k |d_k c_k| + BG + |dd zn|)),   BG = |dr| + |dg| + |db|
  A        = G T:           e(A) = ONE (e(G) T + |G| e(T) + u |A|) + e(G) e(T)
  S        t_i = fl(G_i w_i): e(t) = ONE (e(G) |w| + |G| e(w) + u |t|) + e(G) e(w);  prefix in fp64, total - prefix in fp64, rounded once:
           e(S_j) = sum_{i>j} e(t_i) + u |S_j| + (S + 2) 2^-53 sum_i |t_i|   (total and prefix are S fp64 additions in any order; behind an
           opaque sample S_j is their small difference)
  B        = S / q^:        e(B) = e(S) / q + |B| rho / (1 - rho) + 5 u |B|           (rho < 1/2, else no bound: inf)
  dm       = -A + B:        e(dm) = e(A) + e(B) + u (|A| + |B|)      -- the magnitudes |G_j| T_j + sum_{i>j} |G_i| w_i / q_j, not |dm|: A and B cancel
  F        = delta m:       e(F) = ONE (e(delta) m + |delta| e(m) + u |F|)
  act'     relu: exact, unless x can change sign (|x| <= e(x)): then 1;  identity: exact;
           softplus: 1 / (1 + expf(-x)): (6 + 1 + 5) u + e(x) relative
  dsigma   = (dm F) act':   e = ONE (e(dm) |F| act' + |dm| e(F) act' + |dm F| e(act') + 2 u |dsigma|) + e(dm) e(F) act' + TINY
  dc       = w d_k:         e = ONE (e(w) |d_k| + u |w d_k|) + TINY

  max-blur forward   0.5 (front + rear) + alpha is two roundings in a fixed order and 0.5 * is exact (fusing it into the addition changes
           nothing): the fp32 evaluation of max_blur_expr is THE result, tolerance 0.
  max-blur backward  the shares 1 / 0.5 / 0 of a maximum are exact; the (at most four) halves of upstream gradients are added in an order the
           specification does not fix: 4 u sum |terms|, and 0 where every sum is exact (integer gradients).
  getBounds          sat_j = fl(sum_{i<j} w_i in fp64): u |sat_j| + C 2^-52 sum |w|;  bounds = sat[en] - sat[st]:
                     e = ONE (u (A_en + A_st) + u |bounds|) + 2 C 2^-52 A_C,   A_j = sum_{i<j} |w_i|
  getBounds backward dw_j = sum_k (+-g_k) over the n_j intervals that cover j, fp32 additions in any order:  ONE (n_j - 1) u sum_k |g_k| [covers]
  dot losses         x = (a0 b0 + a1 b1) + a2 b2: e(x) = ONE 3 u sum_k |a_k b_k|;  f = 1 - x: + u |f|;  f = relu(x): e(x) where x >= -e(x);
                     t = fl(w f): e(t) = ONE (|w| e(f) + u |t|), summed in fp64, times scale in fp64, rounded once:
                     e = |scale| (sum e(t) + M 2^-52 sum |t|) + u |loss|
  dot-loss backward  gs = fl(g scale): u |gs|;  d_w = gs f: ONE (2 u |d_w| + |gs| e(f));  k = (gs w) f'(x), d_a = k b, d_b = k a: 3 roundings, ONE 3 u |.|,
                     plus |gs w b| (|gs w a|) where relu' can flip (|x| <= e(x));  0 where every product is exact (small dyadic inputs).

LEGAL RANGE of getBounds' `below`: 0 ... C - 1 (what searchsorted - 1 of the resampling kernels produces and the reference's torch.gather
accepts: sat has C + 1 entries and en = below + 1).  Sorted or not: the reference never sorts it."""
import torch
import torch.nn.functional as F

from ref_forward_ref import DIV_C, EXP_C, LOG1P_C, SQRT_C, TINY, U

ACT_RELU, ACT_IDENTITY, ACT_SOFTPLUS = 0, 1, 2          # nerf_amd.ops.ACT_*
ONE = 1.01
E_NRM = (1.5 + SQRT_C) * U
F64, F32 = torch.float64, torch.float32
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the comparator
def worst(got, want, tol):
    """max over every element of |got - want| / tol.  A NaN or inf in got, a non-finite want or tol (a bound that says nothing) and any
    error against a zero tolerance are violations: inf."""
    got, want, tol = got.detach().cpu().double(), want.detach().cpu().double(), torch.as_tensor(tol).detach().cpu().double()
    assert got.shape == want.shape, "shape %s, expected %s" % (tuple(got.shape), tuple(want.shape))
    if got.numel() == 0:
        return 0.0
    tol = tol.expand_as(want)
    err = (got - want).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-320), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, INF)))
    bad = ~torch.isfinite(got) | ~torch.isfinite(want) | ~torch.isfinite(tol) | torch.isnan(ratio)
    return float(torch.where(bad, torch.full_like(ratio, INF), ratio).max())


def violations(got, want):
    """the exact stages: how many elements differ in value (0 == -0), a NaN or inf in got counted too"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, "shape %s %s, expected %s %s" % (tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    return int((~(got == want) | ~torch.isfinite(got)).sum())


# ------------------------------------------------------------------------------------------------ the specification (fp64) and its fp32 emulation
def _act(x, act):
    return F.relu(x) if act == ACT_RELU else (F.softplus(x) if act == ACT_SOFTPLUS else x)


def _act_grad(x, act):
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_SOFTPLUS:
        return torch.where(x > 20.0, torch.ones_like(x), 1.0 / (1.0 + torch.exp(-x)))
    return torch.ones_like(x)


def depth_of_sum(S):
    """the most additions one term of a per-ray sum passes through: the lane's own ceil(S / 64) terms, then six levels across the lanes"""
    return (S + 63) // 64 - 1 + 6


def ray_sum(t, dim=1):
    """sum over the samples of a ray.  fp64: exact to fp64.  fp32: as a wavefront does it -- lane l adds its terms l, l + 64, ..., then
    six halving levels"""
    if t.dtype == F64 or t.shape[dim] == 0:
        return t.sum(dim)
    t = t.movedim(dim, -1)
    S = t.shape[-1]
    pad = (-S) % 64
    if pad:
        t = torch.cat((t, t.new_zeros(t.shape[:-1] + (pad,))), dim=-1)
    t = t.reshape(t.shape[:-1] + (-1, 64))
    v = t[..., 0, :]
    for c in range(1, t.shape[-2]):
        v = v + t[..., c, :]
    n = 64
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def norm3(d):
    return torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def chain(sigma, z, dirs, mul_norm, act, shift, mut=()):
    """sigma -> weights with every intermediate, in sigma's dtype (fp64: the specification; fp32: the emulation).  z (N, >= S): the first S
    columns are read.  `mut`: single-term faults planted by the host test."""
    dt = sigma.dtype
    N, S = sigma.shape
    zn = z[:, :S].to(dt)
    nrm = None
    if mul_norm:
        nrm = norm3(dirs[:, -3:].to(dt))[:, None]
        zn = zn * nrm
    last = torch.full((N, 1), 1e10, dtype=dt)
    if "delta_last_is_previous" in mut and S > 1:
        last = zn[:, -1:] - zn[:, -2:-1]
    delta = torch.cat((zn[:, 1:] - zn[:, :-1], last), dim=-1)
    x = sigma + shift if shift else sigma
    m = torch.exp(-_act(x, act) * delta)
    q = m if "no_floor" in mut else m + 1e-10
    P = torch.cumprod(torch.cat((torch.ones((N, 1), dtype=F64), q.double()), dim=-1), dim=-1)           # the product in fp64, rounded once
    T = (P[:, 1:] if "inclusive_product" in mut else P[:, :-1]).to(dt)
    return {"zn": zn, "nrm": nrm, "delta": delta, "x": x, "m": m, "q": q, "T": T, "w": (1.0 - m) * T}


def _scalar(v, dt):
    return torch.tensor(v, dtype=F32).to(dt)              # a float argument reaches the kernel as fp32


def evaluate(rgbo, z, dirs, mul_norm, white_bkg, act, shift=0.0, near_far=None, normal=None, cam_dir=None, mut=()):
    """NeRF.render in rgbo's dtype -> {"w", "rgb", "depth" (near_far given), "normal_img" (normal given)}"""
    dt = rgbo.dtype
    ch = chain(rgbo[..., 3], z, dirs, mul_norm, act, shift, mut)
    w = ch["w"]
    out = {"w": w, "chain": ch}
    rgb = ray_sum(w[:, :, None] * rgbo[..., :3])
    if white_bkg:
        rgb = rgb + (1.0 - ray_sum(w))[:, None]
    out["rgb"] = rgb
    if near_far is not None:
        near, far = _scalar(near_far[0], dt), _scalar(near_far[1], dt)
        zd = z[:, :w.shape[1]].to(dt) if "depth_term_unscaled" in mut else ch["zn"]
        out["depth"] = (ray_sum(w * zd) - near) / (far - near)
    if normal is not None:
        n, c = normal.to(dt), cam_dir.reshape(-1).to(dt)
        out["normal_img"] = (ray_sum(w * ((n[..., 0] * c[0] + n[..., 1] * c[1]) + n[..., 2] * c[2])) + 1.0) * 0.5
    return out


def _objective(out, d_rgb, d_weights, d_depth):
    dt = out["w"].dtype
    y = torch.zeros((), dtype=dt)
    if d_rgb is not None:
        y = y + (out["rgb"] * d_rgb.to(dt)).sum()
    if d_weights is not None:
        y = y + (out["w"] * d_weights.to(dt)).sum()
    if d_depth is not None:
        y = y + (out["depth"] * d_depth.to(dt)).sum()
    return y


def composite_backward_autograd(rgbo, z, dirs, mul_norm, white_bkg, act, shift, near_far, d_rgb, d_weights, d_depth, dt=F64, mut=()):
    """d(sum of the outputs against their upstream gradients) / d(rgbo), (N, S, 4), by torch.autograd in dt"""
    r = rgbo.detach().to(dt).requires_grad_(True)
    with torch.enable_grad():
        y = _objective(evaluate(r, z, dirs, mul_norm, white_bkg, act, shift, near_far if d_depth is not None else None, mut=mut), d_rgb, d_weights, d_depth)
        g, = torch.autograd.grad(y, r, allow_unused=True)
    return torch.zeros_like(r) if g is None else g


def upstream(ch, rgb, d_rgb, d_weights, d_depth, white_bkg, near_far, mut=()):
    """G_j = dL/dw_j as the backward kernel forms it, in the chain's dtype"""
    dt = ch["w"].dtype
    G = torch.zeros_like(ch["w"])
    if d_weights is not None:
        G = G + d_weights.to(dt)
    if rgb is not None and d_rgb is not None:
        d = d_rgb.to(dt)
        dr, dg, db = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        bg = ((dr + dg) + db) if (white_bkg and "no_white_in_G" not in mut) else torch.zeros_like(dr)
        G = G + (((dr * rgb[..., 0] + dg * rgb[..., 1]) + db * rgb[..., 2]) - bg)
    if d_depth is not None:
        dd = d_depth.to(dt)
        if "depth_not_divided" not in mut:
            dd = dd / (_scalar(near_far[1], dt) - _scalar(near_far[0], dt))
        G = G + dd[:, None] * ch["zn"]
    return G


def composite_backward_formula(rgbo, z, dirs, mul_norm, white_bkg, act, shift, near_far, d_rgb, d_weights, d_depth, dt=F64, mut=()):
    """the same gradient by the hand-derived adjoint the kernel implements (suffix sum), in dt; the prefix of G w in fp64 as in the kernel"""
    r = rgbo.detach().to(dt)
    ch = chain(r[..., 3], z, dirs, mul_norm, act, shift)
    G = upstream(ch, r[..., :3], d_rgb, d_weights, d_depth, white_bkg, near_far, mut)
    t = G * ch["w"]
    P = torch.cumsum(t.double(), dim=-1)
    suffix = (P[:, -1:] - P).to(dt)
    if "suffix_inclusive" in mut:
        suffix = suffix + t
    dm = -G * ch["T"] + suffix / ch["q"]
    xg = r[..., 3] if "act_grad_unshifted" in mut else ch["x"]
    ds = dm * (-ch["delta"] * ch["m"]) * _act_grad(xg, act)
    dc = ch["w"][:, :, None] * d_rgb.to(dt)[:, None, :] if d_rgb is not None else torch.zeros_like(r[..., :3])
    return torch.cat((dc, ds[..., None]), dim=-1)


def as_rgbo(sigma):
    """sigma (N, S) as the density column of an all-zero colour record: sigma_to_weights is compositing without colours"""
    return torch.cat((torch.zeros(sigma.shape + (3,), dtype=sigma.dtype), sigma[..., None]), dim=-1)


# ------------------------------------------------------------------------------------------------ the bounds
def _excl_cumsum(t):
    return torch.cumsum(t, dim=-1) - t


def chain_bounds(sigma, z, dirs, mul_norm, act, shift):
    """-> (fp64 chain, {name: e(name)}) for zn, delta, m, q (as rho), T, w"""
    ch = chain(sigma.double(), z, dirs, mul_norm, act, shift)
    zn, delta, x, m, q, T, w = (ch[k] for k in ("zn", "delta", "x", "m", "q", "T", "w"))
    S = zn.shape[1]
    if mul_norm:
        e_zn = ONE * (E_NRM + U) * zn.abs()
        e_delta = ONE * ((E_NRM + 2 * U) * delta.abs() + U * torch.cat((zn[:, 1:].abs() + zn[:, :-1].abs(), zn[:, :1] * 0), dim=-1))
    else:
        e_zn = torch.zeros_like(zn)
        e_delta = U * delta.abs()
    e_delta = torch.cat((e_delta[:, :-1], torch.zeros_like(e_delta[:, -1:])), dim=-1)                    # 1e10 is exact
    e_x = U * x.abs() if shift else torch.zeros_like(x)
    dens = _act(x, act)
    if act == ACT_RELU:
        e_dens = e_x * (x >= -e_x)
    elif act == ACT_SOFTPLUS:
        e_dens = torch.sigmoid(x + e_x) * e_x + (EXP_C + LOG1P_C) * U * dens + 2.1e-9 * ((x - 20.0).abs() <= e_x) * (e_x > 0)
    else:
        e_dens = e_x
    a = dens * delta
    e_a = ONE * (e_dens * delta.abs() + dens.abs() * e_delta + U * a.abs()) + e_dens * e_delta
    hi, lo = torch.exp(-(a - e_a)), torch.exp(-(a + e_a))
    e_m = torch.maximum(hi - m, m - lo) + EXP_C * U * hi + TINY
    e_alpha = e_m + U * (1.0 - m).abs()
    e_q = e_m + U * 1e-10 + U * q
    rho = e_q / q
    e_T = T * (torch.expm1(_excl_cumsum(rho)) + U + S * 2.0 ** -52) + TINY
    e_w = ONE * (e_alpha * T + (1.0 - m).abs() * e_T + U * w.abs()) + e_alpha * e_T + TINY
    return ch, {"zn": e_zn, "delta": e_delta, "x": e_x, "m": e_m, "rho": rho, "T": e_T, "w": e_w}


def _sum_bound(t_abs, e_t, S):
    return e_t.sum(1) + ONE * depth_of_sum(S) * U * (t_abs + e_t).sum(1)


def composite_ref(rgbo, z, dirs, mul_norm, white_bkg, act, shift=0.0, near_far=None, normal=None, cam_dir=None):
    """-> {name: (want, tol)} for "w", "rgb" and, when asked for, "depth" and "normal_img" """
    r = rgbo.double()
    S = r.shape[1]
    want = evaluate(r, z, dirs, mul_norm, white_bkg, act, shift, near_far, normal, cam_dir)
    ch, e = chain_bounds(rgbo[..., 3], z, dirs, mul_norm, act, shift)
    w, e_w = ch["w"], e["w"]
    res = {"w": (w, e_w)}
    c = r[..., :3]
    t = (w[:, :, None] * c).abs()
    tol = _sum_bound(t, ONE * (e_w[:, :, None] * c.abs() + U * t), S)
    if white_bkg:
        e_bg = _sum_bound(w.abs(), e_w, S) + U * (1.0 - w.sum(1)).abs()
        tol = tol + e_bg[:, None] + U * want["rgb"].abs()
    res["rgb"] = (want["rgb"], tol)
    if near_far is not None:
        near, far = _scalar(near_far[0], F64), _scalar(near_far[1], F64)
        zn = ch["zn"]
        t = (w * zn).abs()
        e_acc = _sum_bound(t, ONE * (e_w * zn.abs() + w.abs() * e["zn"] + U * t), S)
        acc = (w * zn).sum(1)
        res["depth"] = (want["depth"], (e_acc + U * (acc - near).abs()) / (far - near).abs() + ONE * (1.0 + DIV_C) * U * want["depth"].abs())
    if normal is not None:
        n, cd = normal.double(), cam_dir.reshape(-1).double()
        dot, dot_abs = (n * cd).sum(-1), (n * cd).abs().sum(-1)
        e_dot = ONE * 3 * U * dot_abs
        t = (w * dot).abs()
        e_acc = _sum_bound(t, ONE * (e_w * dot.abs() + w.abs() * e_dot + U * t), S)
        res["normal_img"] = (want["normal_img"], 0.5 * (e_acc + U * ((w * dot).sum(1) + 1.0).abs()))
    return res


def sigma_to_weights_ref(sigma, z, dirs, act):
    """nerf_amd.ops.sigma_to_weights: dirs given -> z scaled by |d|.  -> (want, tol)"""
    ch, e = chain_bounds(sigma, z, dirs, dirs is not None, act, 0.0)
    return ch["w"], e["w"]


def composite_backward_ref(rgbo, z, dirs, mul_norm, white_bkg, act, shift, near_far, d_rgb, d_weights, d_depth):
    """-> (want, tol), both (N, S, 4): columns 0..2 dL/dc, column 3 dL/dsigma"""
    want = composite_backward_autograd(rgbo, z, dirs, mul_norm, white_bkg, act, shift, near_far, d_rgb, d_weights, d_depth)
    r = rgbo.double()
    ch, e = chain_bounds(rgbo[..., 3], z, dirs, mul_norm, act, shift)
    zn, delta, x, m, q, T, w = (ch[k] for k in ("zn", "delta", "x", "m", "q", "T", "w"))
    G = upstream(ch, r[..., :3], d_rgb, d_weights, d_depth, white_bkg, near_far)
    zero = torch.zeros_like(w)
    a_dw = d_weights.double().abs() if d_weights is not None else zero
    a_col, a_bg, a_dep, e_dep = zero, zero, zero, zero
    if d_rgb is not None:
        d = d_rgb.double()
        a_col = (d[:, None, :] * r[..., :3]).abs().sum(-1)
        if white_bkg:
            a_bg = d.abs().sum(-1, keepdim=True).expand_as(w)
    if d_depth is not None:
        dd = d_depth.double() / (_scalar(near_far[1], F64) - _scalar(near_far[0], F64))
        a_dep = (dd[:, None] * zn).abs()
        e_dep = (2.0 + DIV_C) * U * a_dep + dd.abs()[:, None] * e["zn"]
    e_G = ONE * (3 * U * a_col + 2 * U * a_bg + e_dep + 4 * U * (a_dw + a_col + a_bg + a_dep))
    A = G * T
    e_A = ONE * (e_G * T + G.abs() * e["T"] + U * A.abs()) + e_G * e["T"]
    t = G * w
    e_t = ONE * (e_G * w.abs() + G.abs() * e["w"] + U * t.abs()) + e_G * e["w"]
    suffix = lambda v: v.sum(1, keepdim=True) - torch.cumsum(v, dim=-1)
    Sj = suffix(t)
    e_S = suffix(e_t).clamp_min(0) + U * Sj.abs() + (t.shape[1] + 2) * 2.0 ** -53 * t.abs().sum(1, keepdim=True)
    B = Sj / q
    rho = e["rho"]
    e_B = e_S / q + B.abs() * torch.where(rho < 0.5, rho / (1.0 - rho), torch.full_like(rho, INF)) + DIV_C * U * B.abs()
    e_B = torch.where((Sj == 0) & (e_S == 0), torch.zeros_like(e_B), e_B)                               # (nothing behind the last sample)
    dm = -A + B
    e_dm = e_A + e_B + U * (A.abs() + B.abs())
    Fm = delta * m
    e_F = ONE * (e["delta"] * m + delta.abs() * e["m"] + U * Fm.abs())
    ag = _act_grad(x, act)
    if act == ACT_RELU:
        flip = x.abs() <= e["x"]
        e_ag = flip.double() * (e["x"] > 0)
    elif act == ACT_SOFTPLUS:
        e_ag = ag * ((EXP_C + 1.0 + DIV_C) * U + e["x"])
    else:
        e_ag = zero
    ds = dm * Fm * ag
    tol_s = ONE * (e_dm * Fm.abs() * ag + dm.abs() * e_F * ag + (dm * Fm).abs() * e_ag + 2 * U * ds.abs()) + e_dm * e_F * ag + TINY
    if d_rgb is not None:
        wd = (w[:, :, None] * d_rgb.double()[:, None, :]).abs()
        tol_c = ONE * (e["w"][:, :, None] * d_rgb.double().abs()[:, None, :] + U * wd) + TINY
    else:
        tol_c = torch.zeros_like(r[..., :3])
    return want, torch.cat((tol_c, tol_s[..., None]), dim=-1)


def sigma_to_weights_backward_ref(sigma, z, dirs, act, d_weights):
    want, tol = composite_backward_ref(as_rgbo(sigma), z, dirs, dirs is not None, False, act, 0.0, None, None, d_weights, None)
    return want[..., 3], tol[..., 3]


# ------------------------------------------------------------------------------------------------ max-blur
def max_blur_expr(w, alpha):
    """tests/torch_spec.py max_blur_expr"""
    mx = torch.maximum(w[..., :-1], w[..., 1:])
    return 0.5 * (torch.cat((w[..., :1], mx), dim=-1) + torch.cat((mx, w[..., -1:]), dim=-1)) + alpha


def max_blur_ref(w, alpha):
    """the exact stage: the fp32 evaluation, tolerance 0"""
    return max_blur_expr(w.float(), alpha)


def max_blur_backward(w, g, dt=F64, mut=()):
    x = w.detach().to(dt).requires_grad_(True)
    if "tie_to_one_side" in mut:                                   # the larger argument takes everything, the first one on a tie
        a, b = x[..., :-1], x[..., 1:]
        mx = torch.where(a >= b, a, b)
        y = 0.5 * (torch.cat((x[..., :1], mx), dim=-1) + torch.cat((mx, x[..., -1:]), dim=-1))
    else:
        y = max_blur_expr(x, 0.0)
    return torch.autograd.grad(y, x, g.to(dt))[0]


def max_blur_backward_ref(w, g):
    """-> (want, tol): the halves of upstream gradients one element collects, added in any order"""
    return max_blur_backward(w, g), 4 * U * max_blur_backward(w, g.abs())


# ------------------------------------------------------------------------------------------------ getBounds
def bounds_expr(w, below, mut=()):
    """tests/torch_spec.py bounds_expr; the prefix sum in fp64 rounded once, as the kernel's"""
    sat = torch.cat((torch.zeros((w.shape[0], 1), dtype=w.dtype), torch.cumsum(w.double(), dim=-1).to(w.dtype)), dim=-1)
    en = below[:, 1:] if "end_without_plus_one" in mut else below[:, 1:] + 1
    return torch.gather(sat, -1, en) - torch.gather(sat, -1, below[:, :-1])


def get_bounds_ref(w, below):
    C = w.shape[1]
    assert int(below.min()) >= 0 and int(below.max()) <= C - 1, "below outside its legal range 0 ... C - 1"
    wd = w.double()
    want = bounds_expr(wd, below)
    A = torch.cat((torch.zeros((w.shape[0], 1), dtype=F64), torch.cumsum(wd.abs(), dim=-1)), dim=-1)
    tol = ONE * U * (torch.gather(A, -1, below[:, 1:] + 1) + torch.gather(A, -1, below[:, :-1]) + want.abs()) + 2 * C * 2.0 ** -52 * A[:, -1:]
    return want, tol


def bounds_cover(below, C, mut=()):
    """coef (N, K-1, C): +1 where st <= j < en, -1 where en <= j < st (indices out of order), else 0"""
    j = torch.arange(C)[None, None, :]
    st, en = below[:, :-1, None], below[:, 1:, None] + (0 if "end_without_plus_one" in mut else 1)
    return ((j >= st) & (j < en)).double() - ((j >= en) & (j < st)).double()


def get_bounds_backward_ref(below, g, C):
    coef = bounds_cover(below, C)
    gd = g.double()
    want = torch.einsum("nkj,nk->nj", coef, gd)
    mag = torch.einsum("nkj,nk->nj", coef.abs(), gd.abs())
    cnt = coef.abs().sum(1)
    return want, ONE * (cnt - 1).clamp_min(0) * U * mag


def get_bounds_backward_emulation(below, g, C, mut=()):
    """as the kernel: every w_j gathers the +-g_k of the intervals that cover it, in fp32 (the other terms are exact zeros)"""
    return (bounds_cover(below, C, mut).float() * g.float()[:, :, None]).sum(1)


# ------------------------------------------------------------------------------------------------ the weighted-dot losses
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def dot_loss(w, a, b, mode, scale, mut=()):
    """scale * sum w f(<a, b>), f = 1 - x (WeightedNormalLoss, mode 0) or relu(x) (BackFaceLoss, mode 1), in w's dtype; the sum in fp64"""
    x = dot3(a, b)
    if mode == 0:
        f = 1.0 - x
    elif "backface_ge" in mut:
        f = torch.where(x >= 0, x, torch.zeros_like(x))
    else:
        f = F.relu(x)
    return ((w * f).double().sum() * float(_scalar(scale, F64))).to(w.dtype)


def _dot_terms(w, a, b, mode):
    w, a, b = w.double().reshape(-1), a.double().reshape(-1, 3), b.double().reshape(-1, 3)
    x = dot3(a, b)
    e_x = ONE * 3 * U * (a * b).abs().sum(-1)
    if mode == 0:
        f = 1.0 - x
        e_f = e_x + U * f.abs()
    else:
        f = F.relu(x)
        e_f = e_x * (x >= -e_x)
    return w, a, b, x, e_x, f, e_f


def dot_loss_ref(w, a, b, mode, scale):
    wd, _, _, _, _, f, e_f = _dot_terms(w, a, b, mode)
    s = float(_scalar(scale, F64))
    t = wd * f
    want = t.sum() * s
    e_t = ONE * (wd.abs() * e_f + U * t.abs())
    return want, abs(s) * (e_t.sum() + wd.numel() * 2.0 ** -52 * t.abs().sum()) + U * want.abs()


def dot_loss_backward(g, w, a, b, mode, scale, dt=F64, mut=()):
    """-> (d_w, d_a, d_b) by the kernel's formula in dt"""
    shape = w.shape
    w, a, b = w.to(dt).reshape(-1), a.to(dt).reshape(-1, 3), b.to(dt).reshape(-1, 3)
    gs = g.to(dt).reshape(()) * _scalar(scale, dt)
    x = dot3(a, b)
    if mode == 0:
        f, fp = 1.0 - x, -torch.ones_like(x)
        if "normal_sign" in mut:
            fp = -fp
    else:
        pos = (x >= 0) if "backface_ge" in mut else (x > 0)
        f, fp = torch.where(pos, x, torch.zeros_like(x)), pos.to(dt)
    k = (gs * w * fp)[:, None]
    return (gs * f).reshape(shape), (k * b).reshape(shape + (3,)), (k * a).reshape(shape + (3,))


def dot_loss_backward_ref(g, w, a, b, mode, scale):
    """-> ((d_w, d_a, d_b), (tol_w, tol_a, tol_b))"""
    want = dot_loss_backward(g, w, a, b, mode, scale)
    wd, ad, bd, x, e_x, f, e_f = _dot_terms(w, a, b, mode)
    gs = (g.double().reshape(()) * float(_scalar(scale, F64))).abs()
    flip = ((x.abs() <= e_x) & (e_x > 0)).double() if mode == 1 else torch.zeros_like(x)
    tol_w = ONE * (2 * U * want[0].double().abs().reshape(-1) + gs * e_f)
    tol_a = ONE * 3 * U * want[1].abs().reshape(-1, 3) + (gs * wd.abs() * flip)[:, None] * bd.abs()
    tol_b = ONE * 3 * U * want[2].abs().reshape(-1, 3) + (gs * wd.abs() * flip)[:, None] * ad.abs()
    return want, (tol_w.reshape(w.shape), tol_a.reshape(a.shape), tol_b.reshape(b.shape))


def dot_loss_inputs(M, seed, dyadic=False):
    """w (M,), a, b (M, 3).  Rows 0 / 1 / 2 (mod 7) have dot products of exactly 0 / +1 / -1; `dyadic`: every entry a multiple of 1/8 below 4 in
    magnitude, so that every product and sum of the backward is exact in fp32"""
    gen = torch.Generator().manual_seed(seed)
    if dyadic:
        w = torch.randint(-16, 17, (M,), generator=gen).float() / 8
        a = torch.randint(-16, 17, (M, 3), generator=gen).float() / 8
        b = torch.randint(-16, 17, (M, 3), generator=gen).float() / 8
    else:
        w = torch.rand(M, generator=gen)
        a = F.normalize(torch.randn(M, 3, generator=gen), dim=-1)
        b = F.normalize(torch.randn(M, 3, generator=gen), dim=-1)
    i = torch.arange(M)
    e = torch.eye(3)
    for r, (va, vb) in enumerate(((e[0], e[1]), (e[2], e[2]), (e[1], -e[1]))):
        a[i % 7 == r], b[i % 7 == r] = va, vb
    return w, a, b


# ------------------------------------------------------------------------------------------------ the input families
FAMILIES = ("randn", "one_sample_mass", "near_empty", "softplus_far_tail", "relu_zeros_ties", "equal_depths", "opaque_prefix")
SS = (1, 2, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024)              # both sides of every chunk edge of the forward (128, 256) and backward (256, 512)
ACTS = ((ACT_RELU, 0.0), (ACT_IDENTITY, 0.0), (ACT_SOFTPLUS, 0.0), (ACT_SOFTPLUS, 0.5))


def ray_inputs(N, S, act, shift=0.0, seed=0, z_extra=0):
    """fp32 inputs of N rays of S samples; ray n belongs to FAMILIES[n % 7]:
      (a) randn: densities randn * 2 on sorted uniform depths in [2, 6) (every other family starts from these);
      (b) one_sample_mass: sigma = 400 on one sample, -5 elsewhere;
      (c) near_empty: act(sigma) * delta ~ 1e-6, the `1 - expf` regime;
      (d) softplus_far_tail: sigma in [-30, -15] on the last three samples (delta = 1e10: exp(-softplus * 1e10) neither 0 nor 1);
      (e) relu_zeros_ties: integer densities -- exact zeros (also sigma = -shift) and equal neighbours;
      (f) equal_depths: two equal consecutive depths, delta = 0, at three places;
      (g) opaque_prefix: sigma = 1e4 on the first 12 samples, T falls by 1e-10 per sample to below the fp32 range.
    The identity activation takes |sigma| (exp(-sigma * 1e10) must stay finite).  -> dict of sigma (N, S), rgb (N, S, 3), rgbo, z (N, S + z_extra: the
    extra columns hold NaN, nothing may read them), dirs (N, 3), rays (N, 6), normal (N, S, 3), cam_dir (3,), d_rgb, d_weights, d_depth"""
    gen = torch.Generator().manual_seed(1000 * S + 10 * act + seed)
    sigma = torch.randn(N, S, generator=gen) * 2.0
    z = torch.sort(torch.rand(N, S, generator=gen) * 4 + 2, dim=-1)[0]
    fam = torch.arange(N) % len(FAMILIES)
    col = torch.arange(S)[None, :]
    pick = torch.randint(0, S, (N, 1), generator=gen)
    rows = lambda k: (fam == k)[:, None]
    sigma = torch.where(rows(1), torch.where(col == pick, torch.tensor(400.0), torch.tensor(-5.0)), sigma)
    dens = (0.5 + torch.rand(N, S, generator=gen)) * 1e-6 * S / 4.0
    sigma = torch.where(rows(2), torch.log(torch.expm1(dens.double())).float() - shift if act == ACT_SOFTPLUS else dens, sigma)
    sigma = torch.where(rows(3) & (col >= S - 3), -15.0 - 15.0 * torch.rand(N, S, generator=gen), sigma)
    sigma = torch.where(rows(4), torch.round(sigma) - shift, sigma)
    if S >= 2:
        for k in range(3):
            j = torch.randint(0, S - 1, (N, 1), generator=gen)
            z = torch.where(rows(5) & (col == j + 1), torch.gather(z, 1, j).expand(N, S), z)
        z = torch.sort(z, dim=-1)[0]
    sigma = torch.where(rows(6) & (col < min(12, S - 1)), torch.tensor(1e4), sigma)
    if act == ACT_IDENTITY:
        sigma = sigma.abs()
    rgb = torch.rand(N, S, 3, generator=gen)
    dirs = torch.randn(N, 3, generator=gen) * 0.3 + torch.tensor([0.0, 0.0, -1.0])
    zw = torch.cat((z, torch.full((N, z_extra), float("nan"))), dim=-1) if z_extra else z
    return {"sigma": sigma, "rgb": rgb, "rgbo": torch.cat((rgb, sigma[..., None]), dim=-1), "z": zw, "dirs": dirs,
            "rays": torch.cat((torch.randn(N, 3, generator=gen), dirs), dim=-1),
            "normal": F.normalize(torch.randn(N, S, 3, generator=gen), dim=-1), "cam_dir": F.normalize(torch.randn(3, generator=gen), dim=0),
            "d_rgb": torch.randn(N, 3, generator=gen), "d_weights": torch.randn(N, S, generator=gen), "d_depth": torch.randn(N, generator=gen),
            "family": fam}


def flags_of(S, k):
    """the flag combination case k of row length S runs with: every flag takes both values over the row lengths and the four activations"""
    i = SS.index(S) + k if S in SS else S + k
    return {"mul_norm": i % 2 == 0, "white_bkg": (i // 2) % 2 == 0, "near_far": (2.0, 6.0) if i % 3 else None, "rays6": i % 4 == 1, "z_extra": (i % 3) * 3}


UPSTREAMS = (("d_rgb",), ("d_weights",), ("d_depth",), ("d_rgb", "d_weights", "d_depth"))


def bounds_inputs(N, C, K, kind, seed=0):
    """w (N, C), below (N, K) in the legal range 0 ... C - 1 with both ends present, g (N, K-1).  kind: sorted / unsorted / constant"""
    gen = torch.Generator().manual_seed(7 * C + K + seed)
    w = torch.rand(N, C, generator=gen)
    below = torch.randint(0, C, (N, K), generator=gen)
    below[:, 0], below[:, -1] = 0, C - 1
    if K > 2:
        below[0, :], below[1 % N, :] = C - 1, 0                     # rows that read only the top / only the bottom of the summed-area row
    if kind == "sorted":
        below = torch.sort(below, dim=-1)[0]
    elif kind == "constant":
        below = torch.randint(0, C, (N, 1), generator=gen).expand(N, K).contiguous()
        below[0, :], below[1 % N, :] = C - 1, 0
    return w, below, torch.randn(N, K - 1, generator=gen)
