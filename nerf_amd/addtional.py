"""Host-side mirror of the reference's ``nerf/addtional.py`` (sic): ProposalNetwork, getBounds and the
scalar losses.  Same names, signatures and ``state_dict`` keys."""
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from . import autograd_bridge as ab
from ._packed import PackedWeightsMixin, require_no_grad
from .nerf_helper import makeMLP


def getBounds(weights: torch.Tensor, inds: torch.Tensor):
    """Proposal weight mass covering each fine interval (addtional.py:14-18, index quirk included)."""
    if ab.needs_grad(weights):
        return ab.HipOp.apply(lambda w, i: ops.get_bounds(w, i), lambda g, w, i: (ops.get_bounds_backward(i, g, w.shape[-1]), None), 1, weights, inds)
    return ops.get_bounds(weights, inds)


class ProposalLoss(nn.Module):
    def forward(self, prop_bounds: torch.Tensor, nerf_weights: torch.Tensor) -> torch.Tensor:
        """sum relu(w - bound)^2 / (w + 1e-8)  (addtional.py:20-24)."""
        return torch.sum(F.relu(nerf_weights - prop_bounds) ** 2 / (nerf_weights + 1e-8))


def _distortion(weights: torch.Tensor, t: torch.Tensor, mode: int, scale: float, expr) -> torch.Tensor:
    """scale * distortion loss on the device: one wavefront per ray + a fixed-order sum forward, one kernel backward
    (nerf_amd_distortion_loss[_backward]); `expr` = the torch expression, the specification (and what CPU tensors evaluate)."""
    if not weights.is_cuda:
        return expr(weights, t) * scale
    if t.shape[-1] > ops.BWD_MAX_SAMPLES:
        ab.unsupported("a distortion loss over rows of %d depths (the kernels stage a ray in LDS: <= %d)" % (t.shape[-1], ops.BWD_MAX_SAMPLES))
    if not ab.needs_grad(weights, t):
        return ops.distortion_loss(weights, t, mode, scale)
    need = (weights.requires_grad, t.requires_grad)
    return ab.HipOp.apply(lambda w_, t_: ops.distortion_loss(w_, t_, mode, scale),
                          lambda g, w_, t_: ops.distortion_loss_backward(g, w_, t_, mode, scale, need), 1, weights, t)


class Regularizer(nn.Module):
    def __init__(self) -> None:
        super().__init__()

    def forward(self, weights: torch.Tensor, fine_ts: torch.Tensor):
        """mean_ij a_i a_j |c_i - c_j| / r_i + mean_i delta_i a_i^2 / 3 over the 2-tap averages a of the weights and the centres c of
        consecutive depths, r_i = || c_i - c ||  (addtional.py:26-35): weights, fine_ts (N, S), rows in any order.  Rows whose centres
        coincide (S = 2 among them) give NaN, like the reference."""
        def expr(weights, fine_ts):
            center = (fine_ts[..., :-1] + fine_ts[..., 1:]) / 2.
            dists = torch.abs(center[:, None, :] - center[..., None])
            dists = dists / dists.norm(dim=-1, keepdim=True)
            avg_weights = (weights[..., :-1] + weights[..., 1:]) / 2.
            delta = fine_ts[..., 1:] - fine_ts[..., :-1]
            return torch.mean(avg_weights[:, None, :] * avg_weights[..., None] * dists) + torch.mean(delta * (avg_weights ** 2)) / 3.
        return _distortion(weights, fine_ts, 0, 1.0, expr)


class DistortionLoss(nn.Module):
    """Mip-NeRF 360's distortion loss L_dist (Barron et al. 2022, eq. 15), not in the reference: for weights w (N, M) of the M intervals
    between sorted edges e (N, M+1) with midpoints m,  scale * mean_rays [ sum_ij w_i w_j |m_i - m_j| + sum_i w_i^2 (e_i+1 - e_i) / 3 ].
    L_dist is 1-homogeneous in the edges: the loss in normalised coordinates s = (e - near) / (far - near) is scale = 1 / (far - near)."""

    def __init__(self, scale: float = 1.0) -> None:
        super().__init__()
        self.scale = float(scale)

    def forward(self, weights: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
        def expr(w, e):
            mid = (e[..., :-1] + e[..., 1:]) / 2.
            pair = (w[..., :, None] * w[..., None, :] * torch.abs(mid[..., :, None] - mid[..., None, :])).sum((-2, -1))
            return torch.mean(pair + (w * w * (e[..., 1:] - e[..., :-1])).sum(-1) / 3.)
        return _distortion(weights, edges, 1, self.scale, expr)


class InterlevelLoss(nn.Module):
    """Mip-NeRF 360's interlevel loss L_prop (Barron et al. 2022, eq. 13), not in the reference: the fine weights w (N, M) over their
    ascending edges t (N, M + 1) are bounded by the proposal mass that geometrically overlaps each fine interval,
    scale * sum relu(w - bound)^2 / (w + 1e-8)  (the sum and eps of ProposalLoss: the two are interchangeable in magnitude).
    ``prop_edges`` holds the K + 1 edges of the K proposal weights, or -- (N, K) -- the K depths of point samples, the last interval then
    open to +inf as get_weights composites it.  Unlike getBounds it needs no bin indices: any histogram can be supervised, not only the
    one the fine samples were drawn from.  ``weights`` is detached; the gradient goes to ``prop_weights`` alone (the loss is piecewise
    constant in the edges)."""

    def __init__(self, scale: float = 1.0) -> None:
        super().__init__()
        self.scale = float(scale)

    @staticmethod
    def bounds(edges: torch.Tensor, prop_weights: torch.Tensor, prop_edges: torch.Tensor) -> torch.Tensor:
        """The specification: bound_i = c[hi(t_i+1)] - c[lo(t_i)] with c the exclusive prefix sum of prop_weights, lo(v) the last
        proposal edge <= v (0 if none) and hi(v) the first one > v (K if none)."""
        K = prop_weights.shape[-1]
        if prop_edges.shape[-1] == K:
            prop_edges = torch.cat((prop_edges, torch.full_like(prop_edges[..., :1], float("inf"))), -1)
        c = torch.cat((torch.zeros_like(prop_weights[..., :1]), torch.cumsum(prop_weights, -1)), -1)
        cnt = torch.searchsorted(prop_edges.contiguous(), edges.contiguous(), right=True)              # proposal edges <= each fine edge
        lo = (cnt[..., :-1] - 1).clamp(min=0)
        hi = cnt[..., 1:].clamp(max=K)
        return torch.gather(c, -1, hi) - torch.gather(c, -1, lo)

    def forward(self, weights: torch.Tensor, edges: torch.Tensor, prop_weights: torch.Tensor, prop_edges: torch.Tensor) -> torch.Tensor:
        weights, edges, prop_edges = weights.detach(), edges.detach(), prop_edges.detach()
        if not weights.is_cuda:
            bound = self.bounds(edges, prop_weights, prop_edges)
            return torch.sum(F.relu(weights - bound) ** 2 / (weights + 1e-8)) * self.scale
        if max(weights.shape[-1], prop_weights.shape[-1]) > ops.INTERLEVEL_MAX:
            ab.unsupported("an interlevel loss over rows of %d and %d intervals (the kernels stage a ray's rows in LDS: <= %d)"
                           % (weights.shape[-1], prop_weights.shape[-1], ops.INTERLEVEL_MAX))
        scale = self.scale
        if not ab.needs_grad(prop_weights):
            return ops.interlevel_loss(weights, edges, prop_weights, prop_edges, scale)
        return ab.HipOp.apply(lambda p: ops.interlevel_loss(weights, edges, p, prop_edges, scale),
                              lambda g, p: (ops.interlevel_loss_backward(g, weights, edges, p, prop_edges, scale),), 1, prop_weights)


class SoftL1Loss(nn.Module):
    def __init__(self, epsilon=0.001) -> None:
        super().__init__()
        self.eps = epsilon

    def forward(self, pred: torch.Tensor, target: torch.Tensor):
        """Despite the name: plain MSE (addtional.py:37-42)."""
        return torch.mean((pred - target) ** 2)


class LossPSNR(nn.Module):
    __LOG_10__ = 2.3025851249694824

    def forward(self, x):
        """-10 log10(mse)  (addtional.py:45-51)."""
        return -10. * torch.log(x) / LossPSNR.__LOG_10__


class ProposalNetwork(PackedWeightsMixin, nn.Module):
    _net_id = ops.NET_PROPOSAL
    _supports_grad_sinks = True          # the weight-gradient kernels can write into parallel.FlatGradients views

    @staticmethod
    def init_weight(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def __init__(self, position_flevel, hidden_unit=128, cat_origin=True) -> None:
        super().__init__()
        self.position_dims = position_flevel * 6
        self.position_flevel = position_flevel
        self.cat_origin = cat_origin
        self.hidden_unit = hidden_unit
        in_dim = self.position_dims + (3 if cat_origin else 0)
        self.layers = nn.Sequential(*makeMLP(in_dim, hidden_unit), *makeMLP(hidden_unit, hidden_unit),
                                    *makeMLP(hidden_unit, hidden_unit), *makeMLP(hidden_unit, hidden_unit),
                                    *makeMLP(hidden_unit, 1, None))
        self.apply(self.init_weight)

    def _linear_layers(self):
        return [self.layers[0], self.layers[2], self.layers[4], self.layers[6], self.layers[8]]

    def _check_config(self):
        # position_flevel < 10 / cat_origin=False: the same kernels with zero weights on the encoding columns the module lacks (_packed.py)
        # Shapes LARGER than the compiled ones (`--prop_net_width` above 256, more than 10 octaves): layer by layer on the generic MFMA GEMM
        # (nerf_amd/generic_path.py), forward and backward.
        if not (self.position_flevel >= 1 and self.hidden_unit >= 1):
            raise NotImplementedError("nerf_amd: ProposalNetwork needs position_flevel >= 1 and hidden_unit >= 1")

    def _generic(self) -> bool:
        return self.hidden_unit > 256 or self.position_flevel > 10

    def _column_segments(self):
        if self.position_flevel == 10 and self.cat_origin:
            return None
        return [[self.encoding_segment(self.position_flevel, self.cat_origin)], None, None, None, None]

    def _kernel_weight_shapes(self):
        return [(256, 63), (256, 256), (256, 256), (256, 256), (1, 256)]

    # hidden_unit <= 128 (the class default, addtional.py:61; `--prop_net_width 128`): the narrow-tile kernel on its own packed layout
    # (include/nerf_amd.h NERF_AMD_NET_PROPOSAL_128) for every forward-only call; widths below 128 are zero-padded to it (exact).
    _NARROW_SHAPES = [(128, 63), (128, 128), (128, 128), (128, 128), (1, 128)]

    def _narrow_layout(self) -> bool:
        return self.hidden_unit <= 128

    def _pack_now(self, precision: int, narrow: bool = False) -> torch.Tensor:
        if not narrow:
            return super()._pack_now(precision)
        ws, bs = self.kernel_params(self._NARROW_SHAPES)
        blob = ops.pack_weights(ops.NET_PROPOSAL_128, precision, ws, bs)
        blob._nerf_amd_layout = ops.PROP_W128                      # ops.* OR this into the precision argument of the calls that take the blob
        return blob

    def loadFromFile(self, load_path: str, use_amp=False, other_stuff=None):
        """addtional.py:73-86."""
        save = torch.load(load_path, map_location="cpu")
        own = self.state_dict()
        own.update({k: save["model"][k] for k in own.keys()})
        self.load_state_dict(own)
        if use_amp:
            from apex import amp
            amp.load_state_dict(save["amp"])
        print("NeRF Model loaded from '%s'" % (load_path))
        if other_stuff is not None:
            return [save[k] for k in other_stuff]

    def forward(self, pts: torch.Tensor, encoded_pt: torch.Tensor = None, contract: bool = False) -> torch.Tensor:
        """pts (N,C,3) -> density (N,C), no activation (addtional.py:88-96).  ``encoded_pt`` (a pre-computed
        encoding) is accepted for signature parity and ignored: the kernel encodes in-register.  ``contract`` (not in the reference;
        BASELINE configs[4]): Mip-NeRF 360 scene contraction of the positions before the encoding."""
        self._check_config()
        if self._generic():
            from . import generic_path
            return generic_path.proposal_forward(self, pts, contract=contract)
        prec = ops.current_precision()
        layers = self._layers()
        params = [l.weight for l in layers] + [l.bias for l in layers]
        if ab.needs_grad(pts, *params):
            if pts.numel() == 0:                                         # an empty batch: nothing to launch, zero gradients for every parameter
                return ops.proposal_forward(self.packed(prec), prec, pts.detach(), contract=contract) + sum(q.sum() for q in params) * 0.0
            # the training forward dumps the hidden activations; the backward is hand-written kernels on them:
            #   parameter gradients: fused dgrad chain + MFMA weight gradients (mlp_backward.py);
            #   RefNeRF.get_grad (train.py:165-168 with prop_normal: d density / d position): a dgrad-only chain down to the encoded
            #   position + the encoding's derivative (nerf_amd_density_grad).  The positions get a gradient only there.
            from . import mlp_backward
            held = {}
            # fp8 dumps (ops.set_train_dumps) unless the positions ask for a gradient: the density-gradient chain re-reads the bf16 activations
            tprec = prec if pts.requires_grad else ops.train_precision(prec)
            want_pos = bool(pts.requires_grad)

            def hip(p, *wb):
                out, held["dump"] = ops.proposal_forward_train(self.packed(prec, wide=True), tprec, p, contract=contract)
                return out

            def bwd(g, p, *wb):
                if "dump" not in held:
                    raise RuntimeError("nerf_amd: the activation dump of this forward was already consumed (backward twice over the same graph)")
                if "bwd_blob" not in held:
                    held["bwd_blob"] = self.packed_backward(prec)
                if ab._VJP.inputs_only:                                  # (contracted positions: through the contraction's Jacobian, round 5)
                    gx = ops.density_grad(ops.NET_PROPOSAL, held["bwd_blob"], prec, held["dump"], p.reshape(-1, 3), scale=g.reshape(-1), contract=contract)
                    return (gx.view(p.shape), *[None] * len(wb))
                gx = None
                if ab.POSITION_GRADS and want_pos:                       # d loss / d pts as well (autograd_bridge.POSITION_GRADS)
                    gx = ops.density_grad(ops.NET_PROPOSAL, held["bwd_blob"], prec, held["dump"], p.reshape(-1, 3), scale=g.reshape(-1), contract=contract).view(p.shape)
                sinks = self.grad_sinks()                                # persistent flat gradient buffer (parallel.FlatGradients)?
                direct = sinks is not None and sinks[2]
                kw = wb[:5]
                gW, gb = mlp_backward.proposal_backward(g.reshape(-1), p.reshape(-1, 3), held.pop("dump"), tprec, kw, packed_bwd=held["bwd_blob"],
                                                        out=(sinks[0], sinks[1]) if direct else None)
                if sinks is not None:
                    if not direct:                                       # a second backward in the same step accumulates
                        torch._foreach_add_(list(sinks[0]) + list(sinks[1]), list(gW) + list(gb))
                    return (gx, *[None] * len(wb))
                gW, gb = self.unpad_grads(gW, gb)
                return (gx, *gW, *gb)
            return ab.HipOp.apply(hip, bwd, 1, pts, *params)
        return ops.proposal_forward(self.packed(prec), prec, pts, contract=contract)

    @staticmethod
    def get_weights(density: torch.Tensor, zvals: torch.Tensor, ray_dirs: torch.Tensor = None) -> torch.Tensor:
        """relu(sigma) -> alpha -> exclusive transmittance product; z scaled by |d| when ray_dirs is
        given (addtional.py:100-107)."""
        if ab.needs_grad(density, zvals):
            if ray_dirs is not None:
                zvals = zvals * ray_dirs.norm(dim=-1, keepdim=True)
            if density.shape[-1] > ops.BWD_MAX_SAMPLES:
                ab.unsupported("a differentiable sigma -> weights row of %d samples (the backward kernel keeps a ray in registers: <= %d)" % (density.shape[-1], ops.BWD_MAX_SAMPLES))
            return ab.HipOp.apply(lambda s, z: ops.sigma_to_weights(s, z, None, ops.ACT_RELU),
                                  lambda g, s, z: (ops.sigma_to_weights_backward(s, z, None, ops.ACT_RELU, g), None), 1, density, zvals)
        return ops.sigma_to_weights(density, zvals, ray_dirs, ops.ACT_RELU)
