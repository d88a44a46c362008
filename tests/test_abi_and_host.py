"""CPU-side checks (no GPU, no compute calls): the C-ABI library loads and exports every symbol
include/nerf_amd.h declares with the arity the ctypes binding assumes; host logic of the interface mirror."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    src = open(os.path.join(ROOT, "include", "nerf_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(nerf_amd_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_library_exports_every_declared_symbol():
    from nerf_amd import _lib
    decl = _header_functions()
    assert len(decl) >= 20
    assert set(decl) == set(_lib.SIGNATURES), (set(decl) ^ set(_lib.SIGNATURES))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in decl.items():
        assert hasattr(raw, name), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_struct_layout_matches_header():
    from nerf_amd import _lib
    # 8-byte alignment of the pointer members, 12 floats of pose at the end
    assert ctypes.sizeof(_lib.Samples) == 8 + 8 + 8 + 4 + 4 + 8 * 4 + 4 + 4 + 4 + 4 + 4 + 48 + 4 + 4 + 4 + 8 + 8 + 8
    assert _lib.Samples.M.offset == 8 and _lib.Samples.pts.offset == 16 and _lib.Samples.rays.offset == 32
    assert _lib.Samples.pose.offset == 84 and _lib.Samples.contract.offset == 132      # the flag sits in the former tail padding
    assert _lib.Samples.ipe.offset == 136 and _lib.Samples.ipe_radius.offset == 140 and _lib.Samples.ipe_dir_norm.offset == 144
    assert _lib.Samples.rng_seed.offset == 152 and _lib.Samples.rng_ray_offset.offset == 160


def test_pure_queries_without_gpu():
    from nerf_amd import _lib
    lib = _lib.lib
    assert lib.nerf_amd_version() == 125
    assert lib.nerf_amd_packed_bytes(_lib.NET_PROPOSAL, _lib.BF16) == 432 * 1024 + 1056 * 4
    fold = (128 * 256 + 128) * 4                       # scratch of the bottle_neck -> rgb_layer.0 fold
    assert lib.nerf_amd_packed_bytes(_lib.NET_MIP, _lib.BF16) == 928 * 1024 + 1984 * 4 + fold
    assert lib.nerf_amd_packed_bytes(_lib.NET_MIP, _lib.F32) == 928 * 2048 + 1984 * 4 + fold
    assert lib.nerf_amd_packed_bytes(7, 0) == 0
    assert lib.nerf_amd_render_workspace_bytes(1000, 128) >= 1000 * (64 * 4 + 129 * 4 + 128 * 16 + 24)
    # argument validation happens before any HIP call
    assert lib.nerf_amd_inverse_sample(None, None, None, 4, 2, 8, 1, None, None, None) == -1
    assert b"C" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_positional_encoding(None, -1, 10, None, None) == -1


def test_state_dict_keys_match_reference(golden):
    """Checkpoint ABI: key names and shapes equal the reference modules'."""
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    g = golden("g16_state_dict_abi")
    from nerf_amd.ref_model import RefNeRF
    for name, mod in (("mip", MipNeRF(10, 4, 256)), ("prop", ProposalNetwork(10, 256)), ("prop128", ProposalNetwork(10)),
                      ("ref", RefNeRF(10, 4))):
        sd = mod.state_dict()
        want = g[name]
        assert list(sd.keys()) == [k for k, _ in want]
        assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for _, s in want]


def test_mip_module_param_count_and_order():
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.addtional import ProposalNetwork
    import weights as W
    m, p = MipNeRF(10, 4, 256), ProposalNetwork(10, 256)
    assert sum(x.numel() for x in m.parameters()) == 530052 and sum(x.numel() for x in p.parameters()) == 214017
    m.load_state_dict(W.mip_state("small")); p.load_state_dict(W.proposal_state("small"))
    assert [tuple(l.weight.shape) for l in m._linear_layers()] == [(256, 63), (256, 256), (256, 256), (256, 256), (256, 319),
                                                                   (256, 256), (256, 256), (256, 256), (1, 256), (128, 283), (3, 128)]
    assert [tuple(l.weight.shape) for l in p._linear_layers()] == [(256, 63), (256, 256), (256, 256), (256, 256), (1, 256)]
    with pytest.raises(NotImplementedError):
        MipNeRF(10, 3, 256)._check_config()          # (the reference's own rgb_layer.0 is built for direction_flevel 4, mip_model.py:34)
    ProposalNetwork(10)._check_config()                # class default width 128 (addtional.py:61): zero-padded to the 256-wide kernels
    # shapes LARGER than the compiled ones run layer by layer on the generic MFMA GEMM (nerf_amd/generic_path.py); smaller ones on the fused kernels
    assert ProposalNetwork(10, 320)._generic() and MipNeRF(12, 4, 256)._generic() and MipNeRF(10, 4, 512)._generic()
    assert not ProposalNetwork(10, 256)._generic() and not MipNeRF(8, 4, 200)._generic()


def test_which_forwards_take_the_bf16_rows_route():
    """generic_path._rows_route (round 5): the layer-by-layer networks carry their activations as bf16 rows (nerf_amd_rows_gemm) only when
    nobody differentiates the forward, under bf16 precision, with hidden widths that are multiples of 8 -- everything else stays on the
    fp32-row route (nerf_amd_gemm); train mode never caches a packed layer (PackedWeightsMixin's rule)."""
    from nerf_amd import generic_path as G, ops
    from nerf_amd.mip_model import MipNeRF
    lin = lambda i, o: torch.nn.Linear(i, o)
    assert G._rows_route(ops.BF16, None, [lin(63, 320), lin(320, 512)])
    assert G._rows_route(ops.BF16 | 0x100, None, [lin(63, 320)])                       # layout flags ride in the upper bits of `precision`
    assert not G._rows_route(ops.F32, None, [lin(63, 320)])                             # the fp32 parity mode
    assert not G._rows_route(ops.BF16, {}, [lin(63, 320)])                              # activations kept for a backward
    assert not G._rows_route(ops.BF16, None, [lin(63, 300)])                            # 300 % 8 != 0: no 16-byte row pieces
    G.ROWS_ROUTE = False
    try:
        assert not G._rows_route(ops.BF16, None, [lin(63, 320)])
    finally:
        G.ROWS_ROUTE = True
    m = MipNeRF(10, 4, 320)
    m.__dict__.setdefault("_rows_packed", {})["x"] = 1
    m.invalidate_packed()
    assert not m.__dict__["_rows_packed"]                                               # one invalidation for both packed forms
    m.__dict__["_rows_packed"]["x"] = 1
    m.train()
    assert not m.__dict__["_rows_packed"]                                               # a train() / eval() switch drops the cache
    assert ops._pad(575, 64) == 576 and ops._pad(512, 64) == 512 and ops._pad(3, 256) == 256


def test_host_scalars_and_patching(golden):
    from nerf_amd import utils, procedures
    g = golden("g01_raygen")
    assert torch.equal(utils.pose_spherical(37.0, -30.0, 4.0), g["pose_full"])
    assert list(utils.fov2Focal(0.6911112070083618, (100, 100))) == g["focal_sq"].tolist()
    assert list(utils.fov2Focal((0.6911112070083618, 0.5), (60, 100))) == g["focal_tuple"].tolist()
    pix, coords = utils.randomFromOneImage(g["img"], (1.0, 1.0))
    assert torch.equal(pix, g["pix"]) and torch.equal(coords, g["coords"])
    pix, coords = utils.randomFromOneImage(g["img"], (0.5, 0.5))
    assert torch.equal(pix, g["pix_crop"]) and torch.equal(coords, g["coords_crop"])
    assert procedures.get_patch_size((800, 800)) == (50, (16, 16))
    assert procedures.get_patch_size((100, 120)) == (40, (2, 3))
    assert procedures.get_patch_size((822, 1237)) == (None, None)
    a = procedures.get_parser().parse_args(["-w", "--fine_sample_pnum", "96"])
    assert a.white_bkg and a.fine_sample_pnum == 96 and a.coarse_sample_pnum == 64 and a.near == 2.0 and a.far == 6.0


def test_uniform_draw_order_is_the_references():
    """render_image draws, per tile, (sz,sz,64) then (sz*sz, n+1) from the CPU default generator."""
    from nerf_amd import procedures
    torch.manual_seed(3)
    u1, u2 = procedures._draw_uniforms(100, 100, 16, 50, (2, 2), "cpu", "reference")
    torch.manual_seed(3)
    for t in range(4):
        a = torch.rand((50, 50, 64)).view(-1, 64)
        b = torch.rand((2500, 17))
        assert torch.equal(u1[t * 2500:(t + 1) * 2500], a) and torch.equal(u2[t * 2500:(t + 1) * 2500], b)


def test_lr_scheduler_and_losses(golden):
    from nerf_amd.nerf_base import DecayLrScheduler
    from nerf_amd.addtional import LossPSNR, ProposalLoss, SoftL1Loss
    g = golden("g15_lr")
    sch = DecayLrScheduler(0.01, 0.1, 100000, 3e-4, 500)
    for s, want in zip(g["steps"].tolist(), g["lr"].tolist()):
        assert abs(sch.update_opt_lr(int(s))[1] - want) <= 1e-12
    g14 = golden("g14_train_step")
    assert abs(LossPSNR()(torch.tensor(g14["img_loss"])).item() - g14["psnr"]) <= 1e-5
    assert abs(ProposalLoss()(g14["bounds"], g14["weights"]).item() - g14["prop_loss"]) <= 1e-5 * max(1.0, g14["prop_loss"])
    assert abs(SoftL1Loss()(g14["rendered"], g14["rgb_tgt"]).item() - g14["img_loss"]) <= 1e-7


def test_ipe_is_a_hip_entry_point_without_cpu_path(golden):
    """Row 12: ipe_feature / coneParameters are HIP kernels (nerf_amd_ipe_feature, nerf_amd_cone_parameters); CPU tensors are rejected
    like everywhere else in the product (the CPU restatement lives in oracle/ and is pinned by G12 / G18)."""
    from nerf_amd.mip_methods import coneParameters, ipe_feature
    g = golden("g12_ipe")
    with pytest.raises(RuntimeError, match="HIP device"):
        ipe_feature(g["z"], g["rays"], 6, 0.0015)
    with pytest.raises(RuntimeError, match="HIP device"):
        coneParameters(g["z"], 0.0015)


def _reference_load(path, keys_shapes):
    """What the reference's NeRF.loadFromFile (nerf_base.py:30-42) does with a checkpoint, restated for the checks below: read
    save['model'], strip DDP's "module." prefix, pick the module's own state_dict keys in order -> [(key, tensor)] (KeyError / shape
    mismatch = the reference module could not load the file)."""
    save = torch.load(path, map_location="cpu")
    stripped = {(k[7:] if k.startswith("module") else k): v for k, v in save["model"].items()}
    out = [(k, stripped[k]) for k, _ in keys_shapes]
    assert [tuple(v.shape) for _, v in out] == [tuple(s) for _, s in keys_shapes]
    return save, out


def test_checkpoint_roundtrip_with_reference_modules(tmp_path, golden):
    """Checkpoint ABI: a file written by the reference's saveModel (golden G25: MipNeRF with Adam state and
    extra entries, ProposalNetwork bare -- written by tests/golden/make_golden.py from the real reference) loads into the nerf_amd
    modules, and the files nerf_amd writes have the reference's layout and load the way the reference's loadFromFile reads them (module
    keys and shapes: golden G16)."""
    import gzip
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.nerf_helper import saveModel
    g16 = golden("g16_state_dict_abi")
    ref_files = {}
    for name in ("mip", "prop"):
        ref_files[name] = str(tmp_path / ("a_%s.pt" % name))
        with gzip.open(os.path.join(ROOT, "tests", "golden", "g25_ckpt_%s.pt.gz" % name)) as f, open(ref_files[name], "wb") as o:
            o.write(f.read())
    ref_mip, ref_prop = (torch.load(ref_files[n], map_location="cpu") for n in ("mip", "prop"))
    assert list(ref_mip["model"].keys()) == [k for k, _ in g16["mip"]] and list(ref_prop["model"].keys()) == [k for k, _ in g16["prop"]]
    mine_mip, mine_prop = MipNeRF(10, 4, 256), ProposalNetwork(10, 256)
    opt2 = torch.optim.Adam(list(mine_mip.parameters()), lr=1e-3)
    assert mine_mip.loadFromFile(ref_files["mip"], False, opt2, ["train_cnt", "epoch"]) == [123, 4]
    mine_prop.loadFromFile(ref_files["prop"])
    for k, v in ref_mip["model"].items():
        assert torch.equal(v, mine_mip.state_dict()[k])
    for k, v in ref_prop["model"].items():
        assert torch.equal(v, mine_prop.state_dict()[k])
    assert opt2.state_dict() == ref_mip["optimizer"]
    # and back: the same modules saved by nerf_amd's saveModel -> a file of the reference's layout, entry for entry ...
    saveModel(mine_mip, str(tmp_path / "c_mip.pt"), {"train_cnt": 123, "epoch": 4}, opt=opt2)
    saveModel(mine_prop, str(tmp_path / "c_prop.pt"))
    for name, ref in (("mip", ref_mip), ("prop", ref_prop)):
        mine = torch.load(str(tmp_path / ("c_%s.pt" % name)), map_location="cpu")
        assert list(mine.keys()) == list(ref.keys()) and list(mine["model"].keys()) == list(ref["model"].keys())
        assert all(torch.equal(v, ref["model"][k]) for k, v in mine["model"].items())
        assert {k: v for k, v in mine.items() if k != "model"} == {k: v for k, v in ref.items() if k != "model"}
        # ... which the reference's loader reads back, and so does a DDP-style "module." prefixed one (nerf_base.py:34-38)
        _, got = _reference_load(str(tmp_path / ("c_%s.pt" % name)), g16[name])
        assert all(torch.equal(v, ref["model"][k]) for k, v in got)
    sd = {"module." + k: v for k, v in mine_mip.state_dict().items()}
    torch.save({"model": sd}, str(tmp_path / "b_mip.pt"))
    _, got = _reference_load(str(tmp_path / "b_mip.pt"), g16["mip"])
    assert all(torch.equal(v, mine_mip.state_dict()[k]) for k, v in got)
    m2 = MipNeRF(10, 4, 256)
    m2.loadFromFile(str(tmp_path / "b_mip.pt"))
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in mine_mip.state_dict().items())


def test_coarse_grad_select_without_mask_gather():
    """RefNeRF.coarse_grad_select (ref_model.py:108-117) is written without the boolean-mask gather (data-dependent size = a device
    sync); it must still return exactly what the reference's formulation returns."""
    import torch
    from nerf_amd.ref_model import RefNeRF
    from oracle import nerf_oracle as O
    g = torch.Generator().manual_seed(9)
    n, c, f = 37, 16, 40
    fine = torch.randn(n, c + f, 3, generator=g)
    sort_inds = torch.argsort(torch.rand(n, c + f, generator=g), dim=-1)
    got = RefNeRF.coarse_grad_select(fine, sort_inds, c)
    sel = torch.cat((torch.zeros(n, f, dtype=torch.bool), torch.ones(n, c, dtype=torch.bool)), dim=-1)
    sel = torch.gather(sel, -1, sort_inds)
    assert torch.equal(got, fine[sel].reshape(n, c, -1))
    assert torch.equal(got, O.coarse_grad_select(fine, sort_inds, c))


@pytest.mark.parametrize("width", [64, 128, 200])
def test_narrower_networks_are_zero_padded_to_the_kernel_shapes(width):
    """--prop_net_width / --nerf_net_width < 256: the host side hands the 256-wide kernels the zero-padded tensors, which define the same
    function (checked here with the CPU oracle on the padded state), and un-pads gradients back to the parameters' shapes."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as O
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    torch.manual_seed(width)
    prop, mip = ProposalNetwork(10, width), MipNeRF(10, 4, width)
    with torch.no_grad():
        for m in list(prop.modules()) + list(mip.modules()):
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(4.0); m.bias.normal_(0.0, 0.05)
    prop._check_config(); mip._check_config()
    pts = torch.cat((torch.rand(40, 7, 3) * 2 - 1, torch.randn(40, 7, 3)), -1)
    for net, fwd, x in ((prop, O.proposal_forward, pts[..., :3]), (mip, O.mip_forward, pts)):
        ws, bs = net.kernel_params()
        assert [tuple(w.shape) for w in ws] == [tuple(s) for s in net._kernel_weight_shapes()]
        layers = net._linear_layers()
        names = [k[:-7] for k in net.state_dict().keys() if k.endswith(".weight")]
        by_layer = {id(l): n for n, l in ((n, dict(net.named_modules())[n]) for n in names)}
        padded = {}
        for l, w, b in zip(layers, ws, bs):
            padded[by_layer[id(l)] + ".weight"], padded[by_layer[id(l)] + ".bias"] = w.detach(), b.detach()
            assert torch.equal(w[: l.weight.shape[0], : l.weight.shape[1]], l.weight) and int((w != 0).sum()) == int((l.weight != 0).sum())
        with torch.no_grad():
            a, b_ = fwd(dict(net.state_dict()), x), fwd(padded, x)
        assert (a - b_).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item())
        gW, gb = net.unpad_grads([torch.ones_like(w) for w in ws], [torch.ones_like(b) for b in bs])
        assert [tuple(g.shape) for g in gW] == [tuple(l.weight.shape) for l in layers] and [tuple(g.shape) for g in gb] == [tuple(l.bias.shape) for l in layers]
    assert ProposalNetwork(10, 512)._generic()       # wider than the compiled shapes: the generic layer-by-layer path, not padding


@pytest.mark.parametrize("L,cat,width", [(6, True, 256), (10, False, 256), (4, False, 96), (1, True, 128), (7, False, 200)])
def test_shallow_encodings_and_cat_origin_are_placed_in_the_kernel_columns(L, cat, width):
    """position_flevel < 10 / cat_origin=False (constructor arguments, mip_model.py:15-18, addtional.py:61): the host side places the
    module's encoding columns inside the compiled [x | 10 octaves] layout with zeros elsewhere -- the same function (checked with the CPU
    oracle: the module's own state at (L, cat_origin) == the kernel-shaped state at (10, True)), in the wide and the narrow-tile shapes,
    and gradients come back through the same column runs."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nerf_oracle as O
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    torch.manual_seed(L * 1000 + width)
    prop, mip = ProposalNetwork(L, width, cat_origin=cat), MipNeRF(L, 4, width, cat_origin=cat)
    with torch.no_grad():
        for m in list(prop.modules()) + list(mip.modules()):
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(4.0); m.bias.normal_(0.0, 0.05)
    prop._check_config(); mip._check_config()
    pts = torch.cat((torch.rand(40, 7, 3) * 2 - 1, torch.randn(40, 7, 3)), -1)
    for net, fwd, x, kw in ((prop, O.proposal_forward, pts[..., :3], dict(L=L)), (mip, O.mip_forward, pts, dict(Lp=L))):
        layers = net._linear_layers()
        names = [k[:-7] for k in net.state_dict().keys() if k.endswith(".weight")]
        by_layer = {id(l): n for n, l in ((n, dict(net.named_modules())[n]) for n in names)}
        with torch.no_grad():
            want = fwd(dict(net.state_dict()), x, cat_origin=cat, **kw)
        for shapes in [net._kernel_weight_shapes()] + ([net._NARROW_SHAPES] if width <= 128 else []):
            ws, bs = net.kernel_params(shapes)
            assert [tuple(w.shape) for w in ws] == [tuple(s) for s in shapes]
            padded = {}
            for l, w, b in zip(layers, ws, bs):
                padded[by_layer[id(l)] + ".weight"], padded[by_layer[id(l)] + ".bias"] = w.detach(), b.detach()
                assert int((w != 0).sum()) == int((l.weight != 0).sum())
            with torch.no_grad():
                got = fwd(padded, x)                                  # the kernels' function: 10 octaves behind the raw position
            assert (want - got).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
        ws, bs = net.kernel_params()
        gW, gb = net.unpad_grads([w.detach().clone() for w in ws], [b.detach().clone() for b in bs])
        assert all(torch.equal(g, l.weight) for g, l in zip(gW, layers)) and all(torch.equal(g, l.bias) for g, l in zip(gb, layers))
    with pytest.raises(NotImplementedError):
        MipNeRF(10, 3)._check_config()
    assert ProposalNetwork(11, 64)._generic() and MipNeRF(11, 4)._generic()       # more octaves than compiled: the generic path


# ------------------------------------------------------------------------------------------------ the call surface as a pinned contract (G20)
# reference names the mirror deliberately does not carry, each with the reason (dead code in the reference: no caller in any entry script or module)
NOT_MIRRORED = {
    "addtional.Regularizer": "distortion regulariser without a caller (addtional.py:26-35)",
    "addtional.Regularizer.__init__": "see Regularizer", "addtional.Regularizer.forward": "see Regularizer",
    "utils.generateTestSamples": "debug helper of the reference's __main__ block (utils.py:22-31)",
    "mip_methods.coneMeanCov": "internal step of ipe_feature (mip_methods.py:25-33): fused into nerf_amd_ipe_feature",
    "mip_methods.multFreq": "internal step of ipe_feature (mip_methods.py:35-45): fused into nerf_amd_ipe_feature",
}


def test_call_signatures_match_the_reference(golden):
    """SURVEY 8b as data: golden G20 holds inspect.signature of every public function, class and method of the reference modules the entry
    scripts import (written by tests/golden/make_golden.py from the REAL reference).  Every one of them must exist in the nerf_amd mirror
    with the same parameter names, kinds and defaults IN THE SAME ORDER; the mirror may only append parameters that have defaults
    (e.g. `rng=`, `contract=`), so that every reference call site binds the same way."""
    import importlib
    import sigtools
    want_all = golden("g20_signatures")
    missing, differ = [], []
    for modname in sigtools.MODULES:
        mod = importlib.import_module("nerf_amd." + modname)
        have = sigtools.module_signatures(mod, modname)
        for name, want in want_all[modname].items():
            key = "%s.%s" % (modname, name)
            if key in NOT_MIRRORED:
                continue
            if name not in have:
                # a method the mirror inherits instead of defining (e.g. from a mixin) still counts: resolve it on the class
                if "." in name:
                    cls, meth = name.split(".", 1)
                    obj = getattr(getattr(mod, cls, None), meth, None)
                    rec = sigtools.signature_record(obj) if obj is not None else None
                    if rec is not None and want != "class":
                        if rec and rec[0][0] != "self" and want and want[0][0] == "self":
                            rec = [["self", "POSITIONAL_OR_KEYWORD", None]] + rec        # (bound lookup of a static function drops nothing; guard anyway)
                        have[name] = rec
                if name not in have:
                    missing.append(key)
                    continue
            got = have[name]
            if want == "class" or got == "class":
                if want != got:
                    differ.append((key, want, got))
                continue
            if got[:len(want)] != want or any(p[2] is None and p[1] not in ("VAR_POSITIONAL", "VAR_KEYWORD") for p in got[len(want):]):
                differ.append((key, want, got))
    assert not missing, "reference names without a mirror: %s" % missing
    assert not differ, "signature differences:\n" + "\n".join("%s\n  reference %s\n  mirror    %s" % d for d in differ)
    for key in NOT_MIRRORED:                                   # the exemption list must not rot: every entry names something the reference has
        m, n = key.split(".", 1)
        assert n in want_all[m], key


def test_nerf_shim_package_serves_every_name_the_entry_scripts_import(golden):
    """SURVEY 8b literally: "a package importable as `nerf.*`".  compat/nerf/ holds one two-line re-export per reference module; golden
    G23 (written from the reference's entry scripts by make_golden.py: train.py:12-20, ddp_train.py:17-25, model_average.py:16-27) lists
    every `from nerf.X import name`.  Each must resolve through the shim to the nerf_amd object of the same name, the shim must cover
    every module the scripts import from (a dropped module -- timer -- must fail a test, not a user), and hold no logic."""
    import importlib
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "compat")
    want = golden("g23_entry_imports")
    assert set(want) == {"train.py", "ddp_train.py", "model_average.py"}
    modules = sorted({m for imp in want.values() for m in imp})
    assert "timer" in modules and "procedures" in modules
    for m in modules:
        assert os.path.exists(os.path.join(compat, "nerf", m + ".py")), "compat/nerf/%s.py missing" % m
        body = [l for l in open(os.path.join(compat, "nerf", m + ".py")).read().splitlines() if l.strip() and not l.startswith(("#", '"""'))]
        assert len(body) <= 5 and any("from nerf_amd.%s import *" % m in l for l in body), (m, body)
    # in a fresh interpreter with ONLY the two paths a user adds (no tests/ on sys.path, no `nerf` from anywhere else)
    code = ("import json, importlib, sys\n"
            "want = json.load(open(sys.argv[1]))\n"
            "n = 0\n"
            "for script, imp in want.items():\n"
            "    for m, names in imp.items():\n"
            "        shim, real = importlib.import_module('nerf.' + m), importlib.import_module('nerf_amd.' + m)\n"
            "        assert shim.__file__.startswith(sys.argv[2]), shim.__file__\n"
            "        for name in names:\n"
            "            assert getattr(shim, name) is getattr(real, name), (script, m, name)\n"
            "            n += 1\n"
            "print('resolved', n)\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, compat]))
    r = subprocess.run([sys.executable, "-c", code, os.path.join(root, "tests", "golden", "g23_entry_imports.json"), compat],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "resolved" in r.stdout, r.stderr[-2000:]


def _ws256(b):
    return (b + 255) // 256 * 256


# the closed forms of the three render workspaces, as the C-ABI documented them before their layouts were described once
_WORKSPACE_FORMS = {
    # density (N,64) | z_fine (N, n_fine+1) | rgbo (N, n_fine, 4) | rays (N, 6), + alignment slack + one scalar slot
    "nerf_amd_render_workspace_bytes": lambda N, F: _ws256(N * 64 * 4) + _ws256(N * (F + 1) * 4) + _ws256(N * F * 16) + _ws256(N * 24) + 512,
    # density | s_c | z_c (N,64 each) | z_fine | rgbo | raw depth (N) | rays, + the same 512
    "nerf_amd_render_warped_workspace_bytes": lambda N, F: (3 * _ws256(N * 64 * 4) + _ws256(N * (F + 1) * 4) + _ws256(N * F * 16) + _ws256(N * 4)
                                                            + _ws256(N * 24) + 512),
    # density | z_fine | z_coarse (N,64) | z_all (N, n_fine+64) | rgbo (.., 4) | normals (.., 3), then the unrounded ray table + alignment slack
    "nerf_amd_render_ref_workspace_bytes": lambda N, F: (2 * _ws256(N * 64 * 4) + _ws256(N * (F + 1) * 4) + _ws256(N * (F + 64) * 4)
                                                         + _ws256(N * (F + 64) * 16) + _ws256(N * (F + 64) * 12) + N * 24 + 256),
}


def test_render_workspace_sizes_are_the_documented_closed_forms():
    """The three *_workspace_bytes functions against their closed forms AND against the table recorded from the build before the layouts
    were described once (tests/golden/render_workspace_bytes.json): byte for byte, the + 512 of the plain and warped entries, the
    unrounded N * 24 + 256 tail of the Ref entry and the 0 for N < 0 or n_fine < 1 included."""
    import json
    from nerf_amd import _lib
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "render_workspace_bytes.json")))
    n_checked = 0
    for name, form in _WORKSPACE_FORMS.items():
        for N in (-1, 0, 1, 7, 1000, 640000):
            for F in (0, 1, 128, 1023):
                want = 0 if N < 0 or F < 1 else form(N, F)
                assert table[name]["%d,%d" % (N, F)] == want, (name, N, F)
                assert getattr(_lib.lib, name)(N, F) == want, (name, N, F)
                n_checked += 1
    # ... and the two-round query, recorded before the entry points were folded into one pipeline: density2 | z_mid (N,P each) join the plain
    # parts in front of z_fine, under disparity spacing also s_mid (N,P)
    rounds = "nerf_amd_render_rounds_workspace_bytes"
    for N in (-1, 0, 1, 7, 1000, 640000):
        for F in (0, 1, 128, 1023):
            for P in (3, 64, 256):
                for spacing, one_round in ((0, "nerf_amd_render_workspace_bytes"), (1, "nerf_amd_render_warped_workspace_bytes")):
                    want = 0 if N < 0 or F < 1 else _WORKSPACE_FORMS[one_round](N, F) + (2 + spacing) * _ws256(N * P * 4)
                    assert table[rounds]["%d,%d,%d,%d" % (N, F, P, spacing)] == want, (N, F, P, spacing)
                    assert _lib.lib.nerf_amd_render_rounds_workspace_bytes(N, F, P, spacing) == want, (N, F, P, spacing)
                    n_checked += 1
    assert n_checked == 72 + 144 and sum(len(t) for t in table.values()) == 72 + 144


# the closed forms of the training backward's workspaces, as bwd_kernels.hip typed them by hand before each workspace was described once.
# Launch geometry: 32-sample subtiles up to the end of the last tile (256 samples in bf16, 128 in fp32); a batch of `jobs` products gets
# cu / jobs workgroups per product for the big-accumulator shapes (heavy) and 2 cu / jobs for the others, at most one per subtile, at least 1.
def _bwd_n_sub(bf16, M):
    ts = 256 if bf16 else 128
    return (M + ts - 1) // ts * (ts // 32)


def _bwd_wg(n_sub, jobs, heavy, cu):
    return max(1, min(cu * (1 if heavy else 2) // jobs, n_sub))


def _bwd_prop_form(bf16, M, cu):
    n = _bwd_n_sub(bf16, M)
    w0, w1 = _bwd_wg(n, 3, True, cu), _bwd_wg(n, 1, False, cu)
    return (3 * (_ws256(w0 * 256 * 256 * 4) + _ws256(w0 * 256 * 4)) + _ws256(w1 * 256 * 64 * 4) + _ws256(w1 * 256 * 4)
            + _ws256(w1 * 32 * 256 * 4) + _ws256(w1 * 32 * 4) + 256)


def _bwd_mip_form(bf16, M, cu):
    n = _bwd_n_sub(bf16, M)
    w0, w1, w2, w3 = _bwd_wg(n, 6, True, cu), _bwd_wg(n, 2, False, cu), _bwd_wg(n, 1, True, cu), _bwd_wg(n, 1, False, cu)
    return (6 * (_ws256(w0 * 256 * 256 * 4) + _ws256(w0 * 256 * 4)) + 2 * _ws256(w1 * 256 * 64 * 4) + _ws256(w1 * 256 * 4)
            + _ws256(w2 * 160 * 256 * 4) + _ws256(w2 * 160 * 4) + _ws256(w3 * 32 * 128 * 4) + _ws256(w3 * 128 * 32 * 4)
            + _ws256(128 * 256 * 4) + 256)


def _bwd_ref_form(bf16, M, cu):
    n = _bwd_n_sub(bf16, M)
    w7, w2, w1h, w1 = _bwd_wg(n, 7, True, cu), _bwd_wg(n, 2, False, cu), _bwd_wg(n, 1, True, cu), _bwd_wg(n, 1, False, cu)
    b = _ws256(17 * n * 16 * (1024 if bf16 else 2048)) + _ws256(M * 192 * 4)          # delta dump (17 slots) | d_allin (M, 192)
    b += 14 * (_ws256(w7 * 256 * 256 * 4) + _ws256(w7 * 256 * 4))                      # 2 x 7 hidden products
    b += 2 * _ws256(w2 * 256 * 64 * 4) + _ws256(w2 * 256 * 4)                          # encoding columns
    b += 2 * (_ws256(w2 * 256 * 128 * 4) + _ws256(w2 * 256 * 4)) + 2 * _ws256(w2 * 256 * 64 * 4)   # x bottle-neck, x IDE
    b += _ws256(w1h * 160 * 256 * 4) + _ws256(w1h * 160 * 4) + _ws256(w1 * 32 * 256 * 4) + _ws256(w1 * 32 * 4)
    return b + 512


def test_backward_workspace_sizes_are_the_documented_closed_forms():
    """nerf_amd_weight_grads_workspace_bytes, nerf_amd_ref_backward_workspace_bytes and nerf_amd_density_grad_workspace_bytes against the
    closed forms above AND against the table recorded from the build that still typed them by hand (tests/golden/
    backward_workspace_bytes.json, for 256 compute units: the MI355X's count and what the library assumes without a GPU): byte for byte,
    the + 256 / + 512 alignment slack, the non-zero sizes of an empty batch and the 0 of every refused combination included."""
    import json
    from nerf_amd import _lib
    cu = 256
    if torch.cuda.is_available():                                                      # (another device: the closed forms alone)
        n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
        assert _lib.lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
        cu = int(n_cu.value)
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "backward_workspace_bytes.json")))
    assert "256 compute units" in table.pop("_header")
    recorded = (lambda name, key, want: table[name][key] == want) if cu == 256 else (lambda name, key, want: True)
    nets = (("PROPOSAL", _lib.NET_PROPOSAL), ("MIP", _lib.NET_MIP), ("REF", _lib.NET_REF))
    precisions = (("F32", _lib.F32), ("BF16", _lib.BF16), ("BF16_F8", _lib.BF16_F8))
    n_checked = 0
    for p, pc in precisions:
        bf16, f8 = pc != _lib.F32, pc == _lib.BF16_F8
        for M in (-1, 0, 1, 32, 33, 2048, 2049, 4097, 16384, 65537, 1048576):
            want = 0 if M < 0 or f8 else _bwd_ref_form(bf16, M, cu)                        # (no fp8 dumps for Ref-NeRF)
            assert recorded("nerf_amd_ref_backward_workspace_bytes", "%s,%d" % (p, M), want), (p, M)
            assert _lib.lib.nerf_amd_ref_backward_workspace_bytes(pc, M) == want, (p, M)
            n_checked += 1
            for n, nc in nets:
                # products only: Ref-NeRF's lie in the workspace of nerf_amd_ref_backward
                want = 0 if M < 0 or n == "REF" else (_bwd_prop_form if n == "PROPOSAL" else _bwd_mip_form)(bf16, M, cu)
                assert recorded("nerf_amd_weight_grads_workspace_bytes", "%s,%s,%d" % (n, p, M), want), (n, p, M)
                assert _lib.lib.nerf_amd_weight_grads_workspace_bytes(nc, pc, M) == want, (n, p, M)
                # d_enc (M, 64) + slack; density gradients exist for the proposal and Ref-NeRF networks, without fp8 dumps
                want = 0 if M < 0 or n == "MIP" or f8 else _ws256(M * 64 * 4) + 256
                assert recorded("nerf_amd_density_grad_workspace_bytes", "%s,%s,%d" % (n, p, M), want), (n, p, M)
                assert _lib.lib.nerf_amd_density_grad_workspace_bytes(nc, pc, M) == want, (n, p, M)
                n_checked += 2
    assert n_checked == 33 + 99 + 99 and sum(len(t) for t in table.values()) == 33 + 99 + 99


def test_shapes_whose_launch_exceeds_the_lds_are_refused_before_any_hip_call():
    """A shape is accepted only if the dynamic LDS of the launch it leads to fits the 64 KiB a kernel gets without an opt-in: four rays
    per workgroup x the kernel's per-ray rows.  nerf_amd_resample holds 5 C + 2 K + 1280 floats per ray (5 C + 2 K <= 2816),
    nerf_amd_get_bounds C + 1.  The refusal names LDS; the largest accepted neighbour passes on to the NULL-argument check."""
    from nerf_amd import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(256)                                   # non-NULL, never dereferenced: every call below fails first

    def resample(C, K, density=p):
        return lib.nerf_amd_resample(density, None, p, None, 0.1, p, 6, None, 4, C, K, 0, 0.01, 0, 0, p, None, None, None, None)

    def get_bounds(C, w=p):
        return lib.nerf_amd_get_bounds(w, p, 4, C, 8, p, None)

    for C, K in ((256, 768), (255, 770), (200, 908), (154, 1023), (153, 1024), (64, 1024)):          # the largest K for each C
        assert 4 * 4 * (5 * C + 2 * K + 1280) <= 65536 and (K == 1024 or 4 * 4 * (5 * C + 2 * (K + 1) + 1280) > 65536)
        assert resample(C, K, density=None) == -1 and b"NULL argument" in lib.nerf_amd_last_error(), (C, K)
    for C, K in ((256, 1024), (256, 769), (255, 771), (200, 909), (154, 1024)):
        assert 4 * 4 * (5 * C + 2 * K + 1280) > 65536
        assert resample(C, K) == -1 and b"LDS" in lib.nerf_amd_last_error(), (C, K)
        assert resample(C, K, density=None) == -1 and b"LDS" in lib.nerf_amd_last_error(), (C, K)   # before the pointers are looked at
    assert resample(257, 8) == -1 and b"need 3 <= C <= 256" in lib.nerf_amd_last_error()               # the range message is unchanged
    assert get_bounds(4096) == -1 and b"LDS" in lib.nerf_amd_last_error()
    assert get_bounds(4095, w=None) == -1 and b"NULL argument" in lib.nerf_amd_last_error()
    assert get_bounds(4097) == -1 and b"bad size" in lib.nerf_amd_last_error()
    # the other launchers' limits follow from their layouts and did not move
    assert lib.nerf_amd_inverse_sample(None, p, p, 4, 256, 1024, 1, p, None, None) == -1 and b"NULL argument" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_warped_resample(None, p, p, 6, p, 4, 256, 384, 0, 0.01, _lib.SPACING_DISPARITY, 2.0, 6.0, 0, 0, p, None, None, None, None) == -1
    assert b"NULL argument" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_warped_resample(p, p, p, 6, p, 4, 256, 385, 0, 0.01, _lib.SPACING_DISPARITY, 2.0, 6.0, 0, 0, p, None, None, None, None) == -1
    assert b"LDS" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_merge_depths(None, p, 4, 1984, 64, p, None) == -1 and b"NULL argument" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_merge_depths(p, p, 4, 1985, 64, p, None) == -1 and b"K + C <= 2048" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_merge_depths_order(None, p, None, 4, 960, 64, p, p, None, None) == -1 and b"NULL argument" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_merge_depths_order(p, p, None, 4, 961, 64, p, p, None, None) == -1 and b"K + C <= 1024" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_get_bounds_backward(None, p, 4, 4096, 2048, p, None) == -1 and b"NULL argument" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_get_bounds_backward(p, p, 4, 4096, 2049, p, None) == -1 and b"K <= 2048" in lib.nerf_amd_last_error()
    # sizes whose row length wraps a 32-bit int to something small (K + C = 2^30: 4 (K + C) floats = 0 mod 2^32) are refused like any other
    # oversize shape: the checks compute in size_t
    for K, C in ((2 ** 30 - 64, 64), (2 ** 30 + 448, 64), (2 ** 29, 2 ** 29), (2 ** 31 - 65, 64), (64, 2 ** 31 - 65), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.nerf_amd_merge_depths(p, p, 4, K, C, p, None) == -1 and b"K + C <= 2048" in lib.nerf_amd_last_error(), (K, C)
        assert lib.nerf_amd_merge_depths_order(p, p, None, 4, K, C, p, p, None, None) == -1 and b"K + C <= 1024" in lib.nerf_amd_last_error(), (K, C)
    for K in (2 ** 30, 2 ** 30 + 1024, 2 ** 31 - 1):
        assert lib.nerf_amd_get_bounds_backward(p, p, 4, 64, K, p, None) == -1 and b"K <= 2048" in lib.nerf_amd_last_error(), K
