"""The interlevel loss (Mip-NeRF 360 L_prop, include/nerf_amd.h) for the tests: the fp64 specification (prefix sum + searchsorted,
autograd for the gradient), the brute-force (N, M, K) overlap-mask version it is checked against, and the input generator.  Plain torch
on whatever device the inputs live on; nothing of the package is imported."""
import torch

EPS = 1e-8
# (M, K) of the host comparison and of the device sweep
HOST_SHAPES = ((1, 1), (2, 1), (1, 2), (3, 64), (64, 3), (63, 65), (128, 64), (1023, 1024))
GPU_SHAPES = ((1, 1), (2, 1), (1, 2), (3, 64), (64, 3), (63, 65), (64, 64), (65, 63), (128, 64), (129, 257), (1024, 1024))


def make_inputs(N, M, K, open_form, ties, seed):
    """fp32 (w (N, M), t (N, M + 1), w_prop (N, K), t_prop (N, Kp)), Kp = K (open form: point-sample depths) or K + 1: fine edges sorted
    2 + 4 rand, proposal edges sorted 1.5 + 5 rand, both weight rows rand normalised to sum 1; `ties` copies every second proposal edge
    into the fine row (when more than fit, M + 1 of them spread evenly) and re-sorts, so that fine and proposal edges coincide exactly"""
    g = torch.Generator().manual_seed(seed)
    Kp = K if open_form else K + 1
    t = torch.sort(2.0 + 4.0 * torch.rand(N, M + 1, generator=g), dim=-1)[0]
    t_prop = torch.sort(1.5 + 5.0 * torch.rand(N, Kp, generator=g), dim=-1)[0]
    w = torch.rand(N, M, generator=g)
    w = w / w.sum(-1, keepdim=True)
    w_prop = torch.rand(N, K, generator=g)
    w_prop = w_prop / w_prop.sum(-1, keepdim=True)
    if ties:
        picked = t_prop[:, ::2]
        if picked.shape[1] > M + 1:                                                  # more than fit: M + 1 of them, spread over the whole span
            picked = picked[:, torch.linspace(0, picked.shape[1] - 1, M + 1).round().long()]
        t = t.clone()
        t[:, : picked.shape[1]] = picked
        t = torch.sort(t, dim=-1)[0]
    return w.contiguous(), t.contiguous(), w_prop.contiguous(), t_prop.contiguous()


def _edges(w_prop, t_prop):
    """the K + 1 proposal edges: +inf appended in the open form"""
    if t_prop.shape[-1] == w_prop.shape[-1]:
        return torch.cat((t_prop, torch.full_like(t_prop[..., :1], float("inf"))), -1)
    assert t_prop.shape[-1] == w_prop.shape[-1] + 1
    return t_prop


def spec_bounds(t, w_prop, t_prop):
    """bound_i = c[hi(t_i+1)] - c[lo(t_i)], c the exclusive prefix sum of w_prop: differentiable in w_prop, in the dtype of w_prop"""
    K = w_prop.shape[-1]
    e = _edges(w_prop, t_prop)
    c = torch.cat((torch.zeros_like(w_prop[..., :1]), torch.cumsum(w_prop, -1)), -1)
    cnt = torch.searchsorted(e.contiguous(), t.contiguous(), right=True)              # #{j : e_j <= t_i}
    lo = (cnt[..., :-1] - 1).clamp(min=0)                                            # max{j : e_j <= t_i}, 0 if none
    hi = cnt[..., 1:].clamp(max=K)                                                   # min{j : e_j > t_i+1}, K if none
    return torch.gather(c, -1, hi) - torch.gather(c, -1, lo)


def brute_bounds(t, w_prop, t_prop):
    """the same bound from the (N, M, K) mask of proposal intervals [e_j, e_j+1) that overlap or touch the fine interval [t_i, t_i+1]"""
    e = _edges(w_prop, t_prop)
    mask = (t[:, :-1, None] < e[:, None, 1:]) & (t[:, 1:, None] >= e[:, None, :-1])
    return (mask.to(w_prop.dtype) * w_prop[:, None, :]).sum(-1)


def loss_from_bounds(w, bounds, scale=1.0):
    return scale * torch.sum(torch.relu(w - bounds) ** 2 / (w + EPS))


def evaluate(w, t, w_prop, t_prop, scale=1.0, bounds_fn=spec_bounds, dtype=torch.float64):
    """-> (bounds (N, M), loss (python float), d loss / d w_prop (N, K)), everything in `dtype` on the given (fp32) inputs, the brute
    force in chunks of rays so that its (n, M, K) mask stays below 2^25 elements"""
    w, t, w_prop, t_prop = (x.detach().to(dtype) for x in (w, t, w_prop, t_prop))
    N, M, K = w.shape[0], w.shape[1], w_prop.shape[1]
    step = max(1, (1 << 25) // (M * K)) if bounds_fn is brute_bounds else max(N, 1)
    bounds, grad, loss = torch.empty_like(w), torch.empty_like(w_prop), 0.0
    for s0 in range(0, N, step):
        p = w_prop[s0:s0 + step].clone().requires_grad_(True)
        b = bounds_fn(t[s0:s0 + step], p, t_prop[s0:s0 + step])
        part = loss_from_bounds(w[s0:s0 + step], b, scale)
        grad[s0:s0 + step] = torch.autograd.grad(part, p)[0]
        bounds[s0:s0 + step] = b.detach()
        loss += part.item()
    return bounds, loss, grad
