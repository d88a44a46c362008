"""The reference's training iteration (train.py:151-218, MipNeRF branch of ``run()``) as ONE device-resident step.

The reference draws the pixel indices, the depth jitter and the inverse-CDF uniforms on the CPU generator and copies them to the device
every iteration (utils.py:76,89,115), reads the camera pose on the host and rewrites the optimizer's learning rate from Python.  At its
batch size (512-1024 rays) the iteration is launch- and copy-bound, not compute-bound.  Here the training image's pixel table, the camera
pose, the random-number seed, the Adam step count and the learning rate all live in DEVICE memory and every random number is drawn in
kernels (Philox4x32-10), so the iteration never synchronises with the host -- and can therefore be captured once in a hipGraph and
replayed: 0.9 ms instead of 1.7 ms per 512-ray step on one MI355X (bench.py ``train_step.rays_512_hipgraph``).

    step = TrainStep(prop_net, mip_net, optimizer, image_hw=(800, 800), focal=f, near=2., far=6., ray_num=512)
    step.capture()                                   # optional: hipGraph replay from now on
    for img, pose in loader:                         # img (3,H,W), pose (3,4): device tensors (nerf_amd.dataset keeps the scene in HBM)
        lr_sch.update_opt_lr(cnt, optimizer)         # DecayLrScheduler as in train.py:218 -- picked up through the device-side lr
        loss, img_loss = step(img, pose)             # device scalars; read them (``.item()``) only when logging

Scene mode -- every batch drawn uniformly over ALL training pixels of the scene, which ``CustomDataSet.get_dataset(to_cuda=True)`` holds
in HBM as images (V,3,H,W) / poses (V,3,4): one kernel (``ops.sample_scene_rays``) reads the stack in place, so the step has no
per-iteration input at all:

    step = TrainStep(prop_net, mip_net, optimizer, image_hw=(800, 800), focal=f, near=2., far=6., ray_num=1024, scene=(images, poses))
    step.capture()
    for cnt in range(iterations):
        lr_sch.update_opt_lr(cnt, optimizer)
        loss, img_loss = step()                      # step.ray_index: the (v H + row) W + col of the rays just trained on

Semantics are those of train.py:164-199: proposal forward -> softplus -> get_weights -> maxBlurFilter -> inverseSample(sort) ->
MipNeRF forward -> render -> getBounds -> ProposalLoss + MSE -> backward -> Adam; with a RefNeRF as the fine network the
``is_ref_model`` branch (train.py:176-187: coarse/fine merge, density-gradient normals, normal and back-face losses, and with
``prop_normal`` the proposal network's normals, train.py:165-168).  Random streams: the in-kernel
sampler of ``validSampler(rng="philox")`` and ``ops.philox_uniforms`` for inverseSample's ``u``, both keyed by one device-resident
seed that ``nerf_amd_advance_seed`` replaces at the end of every step.
"""
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import ops
from .addtional import DistortionLoss, InterlevelLoss, ProposalLoss, ProposalNetwork, getBounds
from .mip_methods import maxBlurFilter
from .nerf_base import NeRF
from .optim import Adam
from .utils import _focal_xy, crop_window, inverseSample, randomFromOneImage

_M62 = (1 << 62) - 1


def rank_seed(seed: int, rank: int) -> int:
    """The sampler seed of data-parallel rank ``rank`` in scene mode.  In image mode the ranks see different images; in scene mode equal
    seeds would give every rank the SAME batch.  Rank 0 keeps ``seed`` unchanged; rank r > 0 gets seed XOR m(r) (62 bits), m a bijection
    of [0, 2^62) that fixes 0 (xorshift / odd-multiply rounds) -- so distinct ranks get distinct seeds whatever the seed, and every
    result is below 2^62 when the seed is.  Pure: no process group is consulted."""
    seed, rank = int(seed), int(rank)
    if not 0 <= rank <= _M62:
        raise ValueError("nerf_amd.training.rank_seed: rank must be in [0, 2^62)")
    if rank == 0:
        return seed
    x = rank
    x = ((x ^ (x >> 31)) * 0xBF58476D1CE4E5B9) & _M62         # each step is invertible modulo 2^62 and maps 0 to 0
    x = ((x ^ (x >> 29)) * 0x94D049BB133111EB) & _M62
    x ^= x >> 32
    return (seed & _M62) ^ x


class TrainStep:
    def __init__(self, prop_net, mip_net, optimizer: Adam, image_hw: Tuple[int, int], focal, near: float, far: float, ray_num: int = 512,
                 coarse_pnum: int = 64, fine_pnum: int = 128, crop_xy=(1.0, 1.0), seed: Optional[int] = None, white_bkg: bool = False,
                 prop_normal: bool = False, grad_hook=None, ipe_radius: Optional[float] = None, contract: bool = False, flat_grads=None,
                 *, scene=None, view_ids=None, cameras=None, spacing: str = "linear", prop_loss: str = "reference", prop_rounds: int = 1,
                 prop_pnum: Optional[int] = None, ipe_cov: str = "metric", grad_clip: float = -0.01, distortion: float = 0.0):
        """``grad_hook``: called between ``loss.backward()`` and ``optimizer.step()`` -- the place of ddp_train.py's gradient all-reduce
        (``lambda: parallel.allreduce_gradients([mip_net, prop_net])``).  An iteration with a hook runs eagerly (``capture`` refuses).
        ``ipe_radius`` (BASELINE configs[2]): the fine network encodes the conical frusta between consecutive fine depths with the
        integrated PE (mip_methods.py:15-58) instead of the point PE; ``contract`` (configs[4]): Mip-NeRF 360 scene contraction of every
        sample position (proposal and fine).  Neither has a caller in the reference -- the wiring is the build's own (oracle.render_rays
        states it), parity unpinned.
        ``flat_grads`` (default: built here; ``False`` = ordinary per-tensor autograd gradients; or pass
        ``nerf_amd.parallel.FlatGradients([mip_net, prop_net], optimizer, group=...)``): data-parallel training the native way --
        the weight-gradient kernels write into ONE persistent flat buffer, and between backward and the optimizer step ONE all_reduce
        (RCCL) averages it over the ranks.  Unlike a ``grad_hook`` this is part of the captured iteration: ``capture()`` records the
        collective into the hipGraph (backend nccl), so the replayed iteration keeps its launch-free pace on N GPUs.
        ``grad_clip`` (train.py:119-121,217 `--grad_clip`, negative = off like the reference's default): global-norm clipping between
        backward and the optimizer step, evaluated on the device (no host read: capturable).
        ``distortion`` (BASELINE configs[4]; not in the reference): adds ``distortion * L_dist`` -- Mip-NeRF 360's distortion loss
        (addtional.DistortionLoss) of the fine weights over the fine_pnum + 1 sorted fine depths in the normalised coordinate
        s = (z - near) / (far - near) -- to the MipNeRF branch's loss, differentiated w.r.t. the weights; the term of the last iteration is
        ``self.dist_loss``.  0 (default) leaves the iteration as it is.
        ``scene`` = (images (V,3,H,W), poses (V,3,4)), contiguous fp32 device tensors with (H, W) == ``image_hw`` (not in the reference,
        which trains on one image per iteration): every batch is drawn uniformly over the (cropped) pixels of all V views -- or of the
        views ``view_ids`` (list / CPU tensor: range-checked once here; device int64 tensor: taken as it is) -- by one kernel that reads
        the stack in place, keyed by the step's device seed.  The step then takes no image: ``step()``; ``set_image`` raises; no image
        buffer is allocated; ``self.ray_index`` (ray_num,) int64 holds the drawn (v H + row) W + col of the last iteration.  The step
        keeps references to both tensors (a captured graph holds their addresses): do not free or reallocate them, writing into them in
        place is fine.  With V = 1 the iteration is bit-identical to the image-mode one on that image.  Data-parallel runs: with a
        reducing ``flat_grads`` whose group has more than one rank, the seed becomes ``rank_seed(seed, rank)`` so that the ranks draw
        different batches (rank 0 keeps the seed).
        ``spacing`` (BASELINE configs[4]; not in the reference): "linear" (default) leaves the iteration as it is; "disparity" draws the
        coarse samples and resamples in Mip-NeRF 360's normalised distance s (include/nerf_amd.h): the samplers are called with near = 0,
        far = 1 so that their ``lengths`` are s_c, positions and every weight use the metric depths W(s), inverseSample runs on s_c, and
        L_dist is evaluated on the sorted s_f directly (no 1 / (far - near) rescale).  Needs 0 < near < far.
        ``prop_loss`` (BASELINE configs[4]; not in the reference): "reference" (default) = getBounds + ProposalLoss on the sampler's bin
        indices; "interlevel" = Mip-NeRF 360's L_prop (addtional.InterlevelLoss) between the fine histogram -- the fine weights over the
        fine_pnum + 1 sorted fine depths, the edges of L_dist -- and the proposal histogram -- the proposal weights over the coarse depths,
        the last interval open --, by geometric overlap; under "disparity" both edge rows are the s rows (the warp is monotone).  The term of
        the last iteration is ``self.prop_loss_value`` (written under "interlevel" only: the default iteration launches nothing new).
        ``prop_rounds`` = 2 (needs "interlevel"): Mip-NeRF 360's two proposal rounds from the one proposal network -- round 1 as before
        gives w1 over z_c; ``prop_pnum`` (default ``coarse_pnum``) depths z_2 are resampled from it (sorted; in s under "disparity"), the
        same network is evaluated there and gives w2 over z_2, the fine depths are drawn from (w2, z_2); the loss term is
        L(w_fine, z_f; w1, z_c) + L(w_fine, z_f; w2, z_2).  The two resamplings use disjoint columns of one Philox draw for the step's seed.
        ``ipe_cov`` (BASELINE configs[4]; with ``ipe_radius`` and ``contract`` only): "metric" (default) leaves the iteration as it is --
        the frustum mean is contracted, its covariance stays metric; "contracted" = Mip-NeRF 360's Sigma' = J Sigma J^T (eq. 11-14) in
        the fine network's sample fetch.  The backward is unchanged: the parameters' gradients read the dumped encoding.
        ``cameras`` (needs ``scene``; not in the reference): the views' intrinsics for a real capture -- one ``nerf_amd.camera.Camera``
        shared by all views, a sequence of V of them, or a (V,12) fp32 device table (include/nerf_amd.h) -- principal point, lens
        distortion and focal lengths per view; the sampler kernel reads the table when it RUNS, so ``capture()`` / replay work with it and
        writing into a table of your own in place is seen by the next step.  The step keeps the table alive like ``scene``.  ``focal`` is
        then unused by the sampler; ``ipe_radius`` stays the caller's scalar.  None (default) leaves the iteration as it is.
        ``scene``, ``view_ids``, ``spacing``, ``grad_clip``, ``distortion``, ``prop_loss``, ``prop_rounds``, ``prop_pnum``, ``ipe_cov`` and
        ``cameras`` are keyword-only (their order carries no meaning)."""
        ops.ipe_contract(contract, ipe_radius, ipe_cov, "nerf_amd.training.TrainStep")
        self.ipe_cov = ipe_cov
        if not isinstance(optimizer, Adam) or not optimizer.lr_on_device:
            raise ValueError("nerf_amd.training.TrainStep needs nerf_amd.optim.Adam(..., lr_on_device=True): the step must not read host state")
        self.prop_net, self.mip_net, self.opt = prop_net, mip_net, optimizer
        self.near, self.far, self.ray_num, self.coarse_pnum, self.fine_pnum = float(near), float(far), int(ray_num), int(coarse_pnum), int(fine_pnum)
        self.fx, self.fy = _focal_xy(focal)
        self.white_bkg = bool(white_bkg)
        from .ref_model import RefNeRF
        self.is_ref = isinstance(mip_net, RefNeRF)
        self.ipe_radius, self.contract = (None if ipe_radius is None else float(ipe_radius)), bool(contract)
        if self.is_ref and self.ipe_radius is not None:
            raise NotImplementedError("nerf_amd.training.TrainStep: the integrated PE is wired for the MipNeRF branch (the Ref-NeRF kernel encodes points)")
        from .procedures import _check_spacing
        self.spacing, self.warped = spacing, _check_spacing(spacing, near, far)
        self.distortion = float(distortion)
        if not self.distortion >= 0.0:
            raise ValueError("nerf_amd.training.TrainStep: distortion must be >= 0")
        if self.is_ref and self.distortion > 0.0:
            raise NotImplementedError("nerf_amd.training.TrainStep: the distortion loss is wired for the MipNeRF branch (the Ref-NeRF step's merged "
                                      "sample set has no closed last interval)")
        if prop_loss not in ("reference", "interlevel"):
            raise ValueError("nerf_amd.training.TrainStep: prop_loss must be 'reference' or 'interlevel' (got %r)" % (prop_loss,))
        if prop_rounds not in (1, 2):
            raise ValueError("nerf_amd.training.TrainStep: prop_rounds must be 1 or 2 (got %r)" % (prop_rounds,))
        if prop_rounds == 2 and prop_loss != "interlevel":
            raise ValueError("nerf_amd.training.TrainStep: prop_rounds=2 needs prop_loss='interlevel' (the reference's bound reads the bin "
                             "indices of the one sampler call that produced the fine depths)")
        if prop_pnum is not None and int(prop_pnum) < 1:
            raise ValueError("nerf_amd.training.TrainStep: prop_pnum must be positive")
        if self.is_ref and (prop_loss != "reference" or prop_rounds != 1):
            raise NotImplementedError("nerf_amd.training.TrainStep: the interlevel loss and the second proposal round are wired for the MipNeRF "
                                      "branch (the Ref-NeRF step's merged sample set is a different histogram)")
        self.prop_loss, self.prop_rounds = prop_loss, int(prop_rounds)
        self.prop_pnum = self.coarse_pnum if prop_pnum is None else int(prop_pnum)
        self.prop_normal = bool(prop_normal) and self.is_ref                              # (train.py: prop_normal only acts with a Ref-NeRF)
        dev = next(mip_net.parameters()).device
        H, W = image_hw
        self.image_hw = (int(H), int(W))
        self.scene = None
        self.cameras = None
        if scene is None:
            if cameras is not None:
                raise ValueError("nerf_amd.training.TrainStep: cameras needs scene=(images, poses); a single image is a one-view scene "
                                 "(scene=(img[None], pose[None]))")
            if view_ids is not None:
                raise ValueError("nerf_amd.training.TrainStep: view_ids needs scene=(images, poses)")
            self.image = torch.zeros((3, H, W), dtype=torch.float32, device=dev)         # static inputs of the (captured) step
            self.pose = torch.zeros((3, 4), dtype=torch.float32, device=dev)
        else:
            images, poses = scene
            for t, name in ((images, "images"), (poses, "poses")):
                if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev):
                    raise ValueError("nerf_amd.training.TrainStep: scene %s must be a contiguous fp32 tensor on the networks' device" % name)
            if images.dim() != 4 or images.shape[1] != 3 or poses.dim() != 3 or tuple(poses.shape) != (images.shape[0], 3, 4):
                raise ValueError("nerf_amd.training.TrainStep: scene = (images (V,3,H,W), poses (V,3,4)), got %s and %s"
                                 % (tuple(images.shape), tuple(poses.shape)))
            if tuple(images.shape[2:]) != self.image_hw:
                raise ValueError("nerf_amd.training.TrainStep: image_hw %s is not the scene's %s" % (self.image_hw, tuple(images.shape[2:])))
            self.scene = (images, poses)                                                  # (kept alive: a captured graph holds their addresses)
            self.view_ids = ops.scene_view_ids(view_ids, images.shape[0], dev)
            self.cameras = ops.scene_cameras(cameras, images.shape[0], dev)               # (kept alive like the scene)
            self.ray_index = torch.zeros((self.ray_num,), dtype=torch.int64, device=dev)
            self.image = self.pose = None
        self.crop_xy = tuple(crop_xy)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())                            # torch.manual_seed governs the whole run
        if self.scene is not None and flat_grads is not None and flat_grads is not False:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size(flat_grads.group) > 1:
                seed = rank_seed(seed, dist.get_rank(flat_grads.group))                   # the ranks of a data-parallel run draw different batches
        self.seed = torch.full((1,), seed, dtype=torch.int64, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.img_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.dist_loss = torch.zeros((), dtype=torch.float32, device=dev)
        # L_dist is 1-homogeneous in the depths: in s = (z - near) / (far - near) it is L_dist(z) / (far - near)
        # (disparity spacing: the depths handed to it ARE s)
        self.dist_fn = DistortionLoss(self.distortion / (1.0 if self.warped else self.far - self.near)) if self.distortion > 0.0 else None
        if self.is_ref:                                      # the bottle-neck perturbation keyed by this step's device-resident seed
            mip_net.__dict__["noise_seed_dev"] = self.seed   # (RefNeRF.forward, noise_rng "philox": a replayed graph draws fresh noise)
        self.prop_loss_fn = ProposalLoss()
        self.interlevel_fn = InterlevelLoss() if self.prop_loss == "interlevel" else None
        self.prop_loss_value = torch.zeros((), dtype=torch.float32, device=dev)
        self.grad_hook = grad_hook
        # an explicitly passed FlatGradients is a request for data-parallel averaging; the default one only holds the gradients (ranks of a
        # model-averaging run, model_average.py, train independently: no implicit collective)
        self._reduce = flat_grads is not None and flat_grads is not False
        if flat_grads is None:
            from .parallel import FlatGradients
            owner = mip_net.__dict__.get("_grad_owner")                                   # a second TrainStep over the same networks (centre crop /
            if owner is not None and prop_net.__dict__.get("_grad_owner") is owner and owner.covers([mip_net, prop_net]):
                flat_grads = owner                                                        # full image) shares the buffer the kernels write into
            else:
                flat_grads = FlatGradients([mip_net, prop_net], optimizer)
        self.flat_grads = flat_grads if flat_grads is not False else None
        if self.flat_grads is not None and getattr(self.flat_grads, "_dead", False):
            raise ValueError("nerf_amd.training.TrainStep: the FlatGradients passed in was detached by a newer owner of these modules")
        self.grad_clip = float(grad_clip)
        self.graph = None

    def release(self) -> None:
        """Take this step's device-resident noise key off the Ref-NeRF module again (planted by the constructor): a module that outlives
        its TrainStep -- moved to another device, trained by hand -- draws its bottle-neck noise key from torch's CPU generator as before."""
        net = getattr(self, "mip_net", None)
        if net is not None and getattr(self, "is_ref", False) and net.__dict__.get("noise_seed_dev") is getattr(self, "seed", None):
            net.__dict__.pop("noise_seed_dev", None)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ---------------------------------------------------------------------------------------------------------------- the iteration
    def _body(self):
        near, far = (0.0, 1.0) if self.warped else (self.near, self.far)                  # disparity spacing: the samplers' lengths are s_c
        if self.scene is not None:                                                        # one gather over the whole stack, read in place
            pts, z_c, rgb_tgt, rays, _ = ops.sample_scene_rays(self.scene[0], self.scene[1], self.fx, self.fy, near, far, self.ray_num,
                                                               self.coarse_pnum, seed_dev=self.seed, window=crop_window(*self.image_hw, self.crop_xy),
                                                               view_ids=self.view_ids, index_out=self.ray_index, cameras=self.cameras)
        else:
            pixels, coords = randomFromOneImage(self.image, self.crop_xy)                 # pure indexing on the device (cached table)
            pts, z_c, rgb_tgt, rays = ops.sample_training_rays_dev(pixels, coords, self.pose, self.fx, self.fy, near, far, self.ray_num,
                                                                   self.coarse_pnum, self.seed)        # train.py:160-162
        dirs = rays[:, 3:]
        if self.warped:
            s_c = z_c
            z_c, pts = ops.warp_depths(s_c, self.near, self.far, rays, spacing=self.spacing)           # metric depths and o + z d
        if self.prop_normal:
            pts.requires_grad_(True)                                                                    # train.py:165
        density = self.prop_net.forward(pts, contract=True) if self.contract else self.prop_net.forward(pts)
        if self.prop_normal:
            from .ref_model import RefNeRF
            coarse_grad = -RefNeRF.get_grad(density, pts)                                               # :167-168
        density = F.softplus(density)                                                                   # :169
        prop_w = maxBlurFilter(ProposalNetwork.get_weights(density, z_c, dirs), 0.01)                   # :170-171
        if self.prop_rounds == 2:
            # one draw, split by column: the two resamplings get independent uniforms (not a shared prefix of one stream)
            u12 = ops.philox_uniforms((self.ray_num, self.prop_pnum + self.fine_pnum + 1), seed_dev=self.seed)
            u = u12[:, self.prop_pnum:].contiguous()
            w1, e1 = prop_w, (s_c if self.warped else z_c)
            if self.warped:
                s_c = inverseSample(w1, e1, self.prop_pnum, sort=True, u=u12[:, :self.prop_pnum].contiguous())[0].detach()
                z_c, pts = ops.warp_depths(s_c, self.near, self.far, rays, spacing=self.spacing)
            else:
                z_c = inverseSample(w1, e1, self.prop_pnum, sort=True, u=u12[:, :self.prop_pnum].contiguous())[0].detach()
                pts = NeRF.length2pts(rays, z_c)[..., :3].contiguous()
            density = F.softplus(self.prop_net.forward(pts, contract=True) if self.contract else self.prop_net.forward(pts))
            prop_w = maxBlurFilter(ProposalNetwork.get_weights(density, z_c, dirs), 0.01)               # w2 over z_2: what the fine depths come from
        else:
            u = ops.philox_uniforms((self.ray_num, self.fine_pnum + 1), seed_dev=self.seed)
        if self.warped:                                                                                 # resample in s, back to metric depths
            s_f, below = inverseSample(prop_w, s_c, self.fine_pnum + 1, sort=True, u=u)
            z_f = ops.warp_depths(s_f, self.near, self.far, spacing=self.spacing)[0]
        else:
            z_f, below = inverseSample(prop_w, z_c, self.fine_pnum + 1, sort=True, u=u)                 # :174
        extra = 0.0
        if self.is_ref:                                                                                 # :175-187
            from .ref_model import BackFaceLoss, RefNeRF, WeightedNormalLoss
            samples, z_f, below, sort_ids = NeRF.coarseFineMerge(rays, z_c, z_f, below)
            pos, fine_dir = samples.split((3, 3), dim=-1)                                               # (views: RefNeRF.forward reads `samples` itself)
            pos.requires_grad_(True)
            rgbo, pred_normal = self.mip_net.forward(pos, fine_dir, contract=True) if self.contract else self.mip_net.forward(pos, fine_dir)
            density_grad = -RefNeRF.get_grad(rgbo[..., -1], pos)
            rgbo[..., -1] = F.softplus(rgbo[..., -1] + 0.5)
            # train.py:182 passes mip_net.density_act POSITIONALLY, i.e. into `mul_norm`: the depths are not scaled by |d| and the
            # density activation stays the default ReLU (a no-op after the softplus) -- reproduced, like the oracle's ref_train_step
            rendered, weights, _ = NeRF.render(rgbo, z_f, dirs, self.mip_net.density_act, white_bkg=self.white_bkg)
            extra = 4e-4 * WeightedNormalLoss()(weights, density_grad, pred_normal) + 0.1 * BackFaceLoss()(weights, pred_normal, fine_dir)
            if self.prop_normal:
                picked = RefNeRF.coarse_grad_select(density_grad, sort_ids, self.coarse_pnum)
                extra = extra + 4e-5 * WeightedNormalLoss()(prop_w, picked.detach(), coarse_grad)       # 4e-4 * 0.1 (:198)
        else:
            edges = s_f if self.warped else z_f                  # the fine_pnum + 1 sorted fine depths: the intervals of L_dist
            if self.ipe_radius is not None:                      # the fine_pnum frusta between the fine_pnum + 1 sorted depths
                rgbo = self.mip_net.forward_rays(rays, z_f, self.fine_pnum, ipe_radius=self.ipe_radius, contract=self.contract, ipe_cov=self.ipe_cov)
                z_f = z_f[..., :-1].contiguous()
            else:
                z_f = z_f[..., :-1].contiguous()                                                        # :188
                rgbo = (self.mip_net.forward_rays(rays, z_f, self.fine_pnum, contract=True) if self.contract
                        else self.mip_net.forward(NeRF.length2pts(rays, z_f)))                          # :189-190
            rendered, weights, _ = NeRF.render(rgbo, z_f, dirs, white_bkg=self.white_bkg)               # :191
            if self.dist_fn is not None:
                extra = self.dist_fn(weights, edges)
        if self.interlevel_fn is None:
            bounds = getBounds(prop_w, below)                                                           # :192
        if self.flat_grads is not None:
            self.flat_grads.bind(); self.flat_grads.begin_step()                                        # (the kernels overwrite: no zeroing pass)
        else:
            self.opt.zero_grad(set_to_none=True)
        img_loss = torch.mean((rendered - rgb_tgt) ** 2)                                                # :194 (nn.MSELoss)
        if self.interlevel_fn is None:
            l_prop = self.prop_loss_fn(bounds, weights.detach())
        else:
            l_prop = self.interlevel_fn(weights, edges, prop_w, s_c if self.warped else z_c)
            if self.prop_rounds == 2:
                l_prop = self.interlevel_fn(weights, edges, w1, e1) + l_prop
        loss = l_prop + img_loss + extra                                                                # :196-198
        loss.backward()
        if self._reduce:
            self.flat_grads.all_reduce()                                                                # ddp_train.py:98, as one collective
        if self.grad_hook is not None:
            self.grad_hook()
        if self.grad_clip > 0.0:                                                                        # train.py:217 grad_clip_func
            if self.flat_grads is not None:                                                             # one norm + one scale over the flat buffer
                self.flat_grads.finalize_window()
                flat = self.flat_grads.flat
                flat.mul_(torch.clamp(self.grad_clip / (torch.linalg.vector_norm(flat) + 1e-6), max=1.0))
            else:
                torch.nn.utils.clip_grad_norm_(list(self.mip_net.parameters()) + list(self.prop_net.parameters()), self.grad_clip)
        self.opt.step()
        ops.advance_seed(self.seed)
        self.loss.copy_(loss.detach())
        self.img_loss.copy_(img_loss.detach())
        if self.dist_fn is not None:
            self.dist_loss.copy_(extra.detach())
        if self.interlevel_fn is not None:
            self.prop_loss_value.copy_(l_prop.detach())

    # ---------------------------------------------------------------------------------------------------------------- driving it
    def set_image(self, img: torch.Tensor, pose: torch.Tensor) -> None:
        """img (3,H,W) / (1,3,H,W), pose (3,4) / (1,3,4) -- device tensors; asynchronous device-to-device copies into the step's inputs"""
        if self.scene is not None:
            raise ValueError("nerf_amd.training.TrainStep: a scene-mode step draws from the whole stack and takes no image")
        self.image.copy_(img.reshape(self.image.shape), non_blocking=True)
        self.pose.copy_(pose.reshape(-1)[:12].reshape(3, 4), non_blocking=True)

    def set_crop(self, crop_xy) -> None:
        """train.py:155 switches from the centre crop to the full image after `center_crop_iter` iterations: the pixel table changes
        shape, so a captured graph is dropped (call capture() again; the eager path needs nothing)."""
        crop_xy = tuple(crop_xy)
        if crop_xy != self.crop_xy:
            self.crop_xy = crop_xy
            self.graph = None

    def capture(self, warmup: int = 2) -> None:
        """Run `warmup` eager iterations on the current image (lazy kernel attributes, optimizer state, allocator pools), then record
        the iteration into a hipGraph.  The warm-up iterations are real training steps."""
        if self.grad_hook is not None:
            raise RuntimeError("nerf_amd.training.TrainStep: an iteration with a grad_hook (collective) is not captured; run it eagerly")
        self.prop_net.train(); self.mip_net.train()
        for _ in range(max(1, warmup)):
            self._body()
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        kw = {}
        if self._reduce and torch.distributed.is_available() and torch.distributed.is_initialized():
            if torch.distributed.get_backend(self.flat_grads.group) != "nccl":
                raise RuntimeError("nerf_amd.training.TrainStep: only an RCCL (backend 'nccl') all-reduce can be captured into the hipGraph")
            kw["capture_error_mode"] = "thread_local"                                     # (the process group's watchdog thread polls events meanwhile)
        with torch.cuda.graph(self.graph, **kw):
            self._body()                                                                  # (recorded, not executed)

    def __call__(self, img: Optional[torch.Tensor] = None, pose: Optional[torch.Tensor] = None):
        if img is not None:
            self.set_image(img, pose)
        if self.graph is not None:
            self.opt.sync_lr()                                                            # a scheduler may have rewritten param_groups' lr
            self.graph.replay()
            ops.parameters_changed()                                                      # (the captured Adam launch ran: packed caches are stale)
        else:
            self._body()
        return self.loss, self.img_loss
