"""Gradients in, new parameters out, on the device: adam_kernel / bwd_launch_adam through ops.adam_step and nerf_amd.optim.Adam, and the
global-norm clip of TrainStep(grad_clip=...), against the fp64 specification and the per-element bounds of tests/update_ref.py (derived
there; tests/test_update_ref_host.py runs the SAME check functions over a torch-fp32 emulation on the CPU and shows that they report
every planted fault).  Every element of every output goes through gate(name, max(err / tol), 1.0); the counter, the guard elements and
every bit-for-bit statement go through gate(name, violations, 0).

The kernel: 1, 47, 48, 49 and 97 tensors (one to three tables of 48) of 1 ... 3 * 8192 + 5 elements (the 32 x 256 grid's third pass and
ragged tail) as views at odd offsets into flat buffers with guard elements around every view; five value regimes in every tensor
(generic, fresh state, g = 0, tiny with a subnormal v, cancelling); four scalar sets and three grad_scale values; lr as an argument and
through lr_dev; the fp32 step counter up to its last exact value 2^24; the optimizer class over three steps against the fp64 trajectory.
The training step: an active clip on the flat and the per-tensor path (structure, coefficient, norm, the moments the optimizer formed,
nothing changed upstream), an inactive clip and grad_clip = 0 bit for bit equal to no clip, the Ref-NeRF branch with prop_normal, and a
captured step replayed against eager steps."""
import os
import sys

import pytest
import torch

import update_ref as R
from conftest import gate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 2.0, 6.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")


def _gates(items):
    failed = []
    for name, value, limit in items:            # every figure goes on record before the first assertion fails
        try:
            gate(name, value, limit)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ the kernel
class Device:
    """update_ref.Emulation's interface over nerf_amd.ops.adam_step: one call, all tensors in one list"""

    def __init__(self):
        from nerf_amd import ops
        self.ops = ops

    def adam(self, tab, state, t0, lr, beta1, beta2, eps, grad_scale, lr_dev=None, g=None):
        p, m, v = (x.clone().cuda() for x in state)
        g = (tab.g if g is None else g).clone().cuda()
        step = torch.full((1,), float(t0), dtype=torch.float32, device="cuda")
        dev_lr = None if lr_dev is None else torch.full((1,), float(lr_dev), dtype=torch.float64, device="cuda")
        self.ops.adam_step(tab.views(p), tab.views(g), tab.views(m), tab.views(v), step, lr, beta1, beta2, eps, grad_scale, lr_dev=dev_lr)
        torch.cuda.synchronize()
        return p.cpu(), m.cpu(), v.cpu(), g.cpu(), float(step.item())


@pytest.fixture(scope="module")
def dev():
    return Device()


@pytest.mark.parametrize("count,si,gs", R.kernel_cases())
def test_adam_kernel_against_fp64(dev, count, si, gs):
    _gates(R.kernel_case_gates(dev, count, si, gs))


def test_adam_kernel_at_the_counters_end(dev):
    _gates(R.counter_end_gates(dev))


def test_adam_class_three_steps_against_the_fp64_trajectory():
    """Adam(params, grad_scale=1/3) from fresh state against the fp64 specification iterated on its own fp64 state (the bound propagated
    through the three steps); state_dict() then reports step 3 for every parameter"""
    from nerf_amd.optim import Adam
    params, grads = R.class_inputs()
    ps = [torch.nn.Parameter(p.clone().cuda()) for p in params]
    opt = Adam(ps, lr=R.CLASS_LR, grad_scale=R.CLASS_GS)
    for t in range(R.CLASS_STEPS):
        for p, g in zip(ps, grads[t]):
            p.grad = g.clone().cuda()
        opt.step()
    torch.cuda.synchronize()
    got = [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in ps]
    items = R.class_gates(got, R.class_reference(params, grads))
    sd = opt.state_dict()
    steps = [float(sd["state"][i]["step"]) for i in range(len(ps))]
    items.append(("update Adam(grad_scale=1/3) state_dict(): parameters whose step is not 3", sum(s != R.CLASS_STEPS for s in steps), 0))
    items.append(("update Adam(grad_scale=1/3) state_dict(): parameters missing", abs(len(sd["state"]) - len(ps)), 0))
    _gates(items)


# ------------------------------------------------------------------------------------------------ the training step
def _nets(kind):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import weights as W
    from nerf_amd.addtional import ProposalNetwork
    prop = ProposalNetwork(10, 256)
    prop.load_state_dict(W.proposal_state("small"))
    if kind == "ref":
        from nerf_amd.ref_model import RefNeRF
        net = RefNeRF(10, 4)
        net.load_state_dict(W.ref_state("small"))
    else:
        from nerf_amd.mip_model import MipNeRF
        net = MipNeRF(10, 4, 256)
        net.load_state_dict(W.mip_state("small"))
    return prop.cuda().train(), net.cuda().train()


def _scene():
    sys.path.insert(0, ROOT)
    from oracle import nerf_oracle as O                                      # (test infrastructure: pose / focal only)
    gen = torch.Generator().manual_seed(3)
    img = torch.rand(3, 40, 40, generator=gen).cuda()
    pose = O.pose_spherical(20.0, -30.0, 4.0)[:3].contiguous().cuda()
    return img, pose, O.fov2focal(0.6911112070083618, (40, 40))


class Step:
    """The smallest TrainStep of the suite (40 x 40 image, 96 rays, 32 coarse + 64 fine samples, fp32, seed 1234, fresh Adam state) with
    the two snapshots of every p.grad: `unclipped` from grad_hook (after the backward, before the clip), `clipped` from an optimizer
    pre-step hook registered AFTER the TrainStep was built (after the clip and after FlatGradients' own hook)."""

    def __init__(self, kind="mip", grad_clip=-0.01, flat=True, snapshots=True):
        from nerf_amd.optim import Adam
        from nerf_amd.training import TrainStep
        self.prop, self.net = _nets(kind)
        self.params = list(self.net.parameters()) + list(self.prop.parameters())
        self.opt = Adam(self.params, lr=1e-3, lr_on_device=True)
        self.unclipped = self.clipped = None
        img, pose, focal = _scene()
        self.st = TrainStep(self.prop, self.net, self.opt, (40, 40), focal, NEAR, FAR, ray_num=96, coarse_pnum=32, fine_pnum=64, seed=1234,
                            prop_normal=(kind == "ref"), grad_hook=self._before_clip if snapshots else None,
                            flat_grads=None if flat else False, grad_clip=grad_clip)
        if snapshots:
            self.opt.register_step_pre_hook(self._after_clip)
        self.st.set_image(img, pose)

    def _grads(self):
        assert all(p.grad is not None for p in self.params)
        return [p.grad.detach().clone() for p in self.params]

    def _before_clip(self):
        self.unclipped = self._grads()

    def _after_clip(self, *_):
        self.clipped = self._grads()

    def moments(self, key):
        return [self.opt.state[p][key] for p in self.params]

    def state(self):
        """every parameter, both moments and the loss, as one list of tensors"""
        torch.cuda.synchronize()
        return [p.detach().clone() for p in self.params] + [x.clone() for x in self.moments("exp_avg")] + [x.clone() for x in self.moments("exp_avg_sq")] + \
            [self.st.loss.clone()]


_PROBE = {}


def _probe(kind):
    """the twin with clipping off: its gradients of the first step and n64, their norm in fp64 (computed once per network kind)"""
    if kind not in _PROBE:
        tw = Step(kind, grad_clip=-0.01, flat=True)
        tw.st()
        torch.cuda.synchronize()
        _PROBE[kind] = (tw.unclipped, R.norm64(tw.unclipped))
    return _PROBE[kind]


def _bits_differ(a, b):
    assert len(a) == len(b)
    return sum(int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) for x, y in zip(a, b))


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "per_tensor"])
def test_active_clip(flat):
    """grad_clip = 0.5 n64: checks 1-5 of update_ref.clip_gates on one eager step"""
    twin, n64 = _probe("mip")
    c = 0.5 * n64
    s = Step("mip", grad_clip=c, flat=flat)
    s.st()
    torch.cuda.synchronize()
    _gates(R.clip_gates("update clip MipNeRF %s c=0.5 n64" % ("flat" if flat else "per-tensor"), s.unclipped, s.clipped, c, flat,
                        exp_avg=s.moments("exp_avg"), exp_avg_sq=s.moments("exp_avg_sq"), twin=twin))


def test_active_clip_refnerf_prop_normal():
    """the Ref-NeRF branch with prop_normal on the flat path: the fine network's gradients arrive through autograd -- the ranges a clip
    placed before the window is closed would miss.  Checks 1, 2 and 4 (3 comes with them)."""
    _, n64 = _probe("ref")
    c = 0.5 * n64
    s = Step("ref", grad_clip=c, flat=True)
    assert s.st.is_ref and s.st.prop_normal
    s.st()
    torch.cuda.synchronize()
    _gates(R.clip_gates("update clip Ref-NeRF prop_normal flat c=0.5 n64", s.unclipped, s.clipped, c, True,
                        exp_avg=s.moments("exp_avg"), exp_avg_sq=s.moments("exp_avg_sq")))


@pytest.mark.parametrize("flat", [True, False], ids=["flat", "per_tensor"])
def test_inactive_clip_changes_nothing(flat):
    """grad_clip = 2 n64 (the coefficient clamps to 1) and grad_clip = 0 (off) against grad_clip = -0.01 (off): parameters, both moments
    and the loss after three steps, bit for bit"""
    _, n64 = _probe("mip")
    runs = {}
    for name, c in (("off", -0.01), ("2 n64", 2.0 * n64), ("0", 0.0)):
        s = Step("mip", grad_clip=c, flat=flat, snapshots=False)
        for _ in range(3):
            s.st()
        runs[name] = s.state()
    tag = "update clip MipNeRF %s three steps, bits that differ from grad_clip=-0.01: " % ("flat" if flat else "per-tensor")
    _gates([(tag + "grad_clip = 2 n64", _bits_differ(runs["2 n64"], runs["off"]), 0), (tag + "grad_clip = 0", _bits_differ(runs["0"], runs["off"]), 0)])


def test_clipped_step_replayed_equals_eager():
    """a flat-path step with the active clip: capture() (two eager warm-up steps) and three replays against a twin's five eager steps"""
    _, n64 = _probe("mip")
    c = 0.5 * n64
    g = Step("mip", grad_clip=c, flat=True, snapshots=False)
    g.st.capture(warmup=2)
    for _ in range(3):
        g.st()
    e = Step("mip", grad_clip=c, flat=True, snapshots=False)
    for _ in range(5):
        e.st()
    _gates([("update clip MipNeRF flat c=0.5 n64: 2 eager + 3 replayed steps, bits that differ from 5 eager steps", _bits_differ(g.state(), e.state()), 0),
            ("update clip MipNeRF flat c=0.5 n64: |step counter - 5| after the replays", abs(float(g.opt.state[g.params[0]]["step"]) - 5.0), 0)])
