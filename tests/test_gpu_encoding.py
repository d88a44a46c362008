"""The input encoding of the proposal and fine kernels, and the stand-alone encoders, against fp64 element by element.
tests/encoding_ref.py holds the specification and the derivation of every bound; tests/test_encoding_ref_host.py shows on the CPU that
an fp32 emulation of the kernels' sequences stays inside every bound on exactly these inputs and that fourteen planted faults do not.

  1. the stand-alone encoders -- positional_encoding, encode_rows (fp32 / bf16, normalize, x_stride 3 and 6), ipe_feature (contract off and
     on), cone_parameters, dirs_norm, direction_table (decoded from its documented 64-byte rows) -- at lengths on both sides of their
     tiles, an empty call, a store tail that is no multiple of four floats, and one call with more tiles than the grid;
  2. the encoding slot of proposal_forward_train / mip_forward_train, read through ops.train_dump_rows and the slot map of
     forward_ref.encodings: position columns, direction columns, raw columns within the derived bounds, the padding features exactly
     zero; fp32 and bf16; every sample source; contraction off and on; the integrated PE off, plain and metric; M = one tile - 1, one
     tile + 1 and 3 n_cu tile + 77, split into rays of a ragged (prime) length;
  3. the inference entry points equal the training forward bit for bit on the same ray descriptors (the point descriptors, plain and
     contracted, and the integrated-PE descriptor are already asserted by
     test_gpu_forward_layers.py::test_render_kernels_equal_the_training_forward_bit_for_bit and are not repeated).

Sample sources: mode 0 with pts_stride 3 / 6 (proposal) and 6 / 8 (fine); mode 1 with explicit z and z_stride = S + 3; mode 1 with
z_base + u z_jitter, u a tensor; the same with u = ops.philox_stream(..., strat=True) -- which must equal the oracle's twin, the input of
the bounds -- and then WITHOUT a tensor: the in-kernel draw must leave the same slot, bit for bit; mode 2.  Both training entry points
accept mode 2: their validation (capi.hip check_samples, called by nerf_amd_proposal_forward_train and nerf_amd_mip_forward_train) admits
modes 0, 1 and 2 alike and refuses only the integrated PE outside mode 1 with explicit depths -- so mode 2 is covered for both networks,
with the integrated PE left to the explicit-z source.

Every element goes through gate(name, max(err / tol), 1.0), every exact stage through gate(name, violations, 0)."""
import ctypes
import time

import pytest
import torch

import backward_ref as R
import encoding_ref as E
import forward_ref as F
import test_gpu_forward_layers as TL
from conftest import gate
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

RADIUS = 2.0 / 12.0 ** 0.5 / 55.0
R2 = E.radius_r2(RADIUS)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    from nerf_amd import ops
    from nerf_amd import _lib

    class NS:
        pass
    ns = NS()
    ns.pkg, ns.ops, ns.lib, ns.Samples = nerf_amd, ops, _lib.lib, _lib.Samples
    ns.ids = {"prop": _lib.NET_PROPOSAL, "mip": _lib.NET_MIP, "prop128": _lib.NET_PROPOSAL_128, "mip128": _lib.NET_MIP_128}
    n_cu, is950 = ctypes.c_int(0), ctypes.c_int(0)
    assert ns.lib.nerf_amd_device_info(ctypes.byref(n_cu), ctypes.byref(is950)) == 0
    ns.n_cu = int(n_cu.value)
    ns.nets = {}
    nerf_amd.set_precision("fp32")
    yield ns
    nerf_amd.set_precision("fp32")


def _emit(prefix, worst, exact=()):
    """one gate line per output; every line is written before the first failure is raised"""
    failed = []
    for k in sorted(worst):
        try:
            gate("%s %s %s" % (prefix, k, "violations" if k in exact else "max(err/tol)"), worst[k], 0.0 if k in exact else 1.0)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


def _bit_differences(a, b):
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    if a.dtype == torch.bfloat16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    else:
        a, b = a.float().view(torch.int32), b.float().view(torch.int32)
    return float((a != b).sum()) if a.shape == b.shape else float("inf")


# ------------------------------------------------------------------------------------------------ 1: the stand-alone encoders
GRID_TILES = 256 * 8                       # the stand-alone launchers' grid cap (sample_kernels.hip blocks_for): more tiles than this loop twice


def _points(M, seed):
    return E.point_batch(M, 6, seed, E.FAR_WIDE * 3.0)


@pytest.mark.parametrize("L", [1, 4, 10])
def test_positional_encoding(A, L):
    """pe_kernel: 64-sample tiles, 16-byte stores with a scalar tail (M 6 L is no multiple of 4 at (M, L) = (1, 1), (63, 1), (65, 1)); at
    L = 10 one call of 2048 tiles + 65 samples, so the first workgroups take a second tile"""
    worst = {}
    for M in (0, 1, 63, 64, 65) + ((GRID_TILES * 64 + 65,) if L == 10 else ()):
        x = _points(M, 100 + M)[:, :3].contiguous()
        got = A.ops.positional_encoding(x.cuda(), L)
        assert got.shape == (M, 6 * L)
        E.merge(worst, E.compare({"pe": E.pe(E.Fl(x.double()), L, "direct")}, {"pe": got}))
    _emit("encoding positional_encoding L=%d" % L, worst)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("L", [4, 10])
def test_encode_rows(A, L, normalize, prec):
    """encode_rows_kernel (sincosf of the device library: 4 u; bf16 rows double from octave 0): x_stride 3 and 6, 256 rows per workgroup;
    the bf16 L = 4 case adds one call of 2048 workgroups + 77 rows"""
    P = TL._code(A, prec)
    worst = {"stride": 0.0}
    big = (GRID_TILES * 256 + 77,) if (L == 4 and prec == "bf16" and not normalize) else ()
    for M in (0, 1, 63, 64, 65, 255, 257) + big:
        pts = _points(M, 7 + L + M).cuda()
        wide = pts[:, 3:6] if normalize else pts[:, :3]                          # x_stride 6
        got = A.ops.encode_rows(wide, L, P, normalize)
        ncol = (3 + 6 * L + 7) // 8 * 8
        assert got.shape == (M, ncol) and got.dtype == (torch.bfloat16 if prec == "bf16" else torch.float32)
        worst["stride"] += _bit_differences(A.ops.encode_rows(wide.contiguous(), L, P, normalize), got)      # x_stride 3: the same bits
        g = got.float().cpu()
        E.merge(worst, E.compare(E.encode_rows(wide.cpu(), L, normalize, prec == "bf16"), {"raw": g[:, :3], "pe": g[:, 3: 3 + 6 * L], "pad": g[:, 3 + 6 * L:]}))
    _emit("encoding encode_rows L=%d normalize=%d %s" % (L, normalize, prec), worst, exact=("stride",))


def _ipe_inputs(N, S, contracted):
    rays = E.ray_batch(N, 50 + N + S)
    z = E.depth_rows(rays, S + 1, E.DEPTH_FAMILIES if contracted else E.DEPTH_FAMILIES[:4], 60 + S)
    return E.clear_of_sphere(rays, z)


IPE_SHAPES = ((0, 1), (1, 1), (63, 1), (64, 1), (65, 1), (9, 7), (10, 7), (1, 128), (3, 128))


@pytest.mark.parametrize("contracted", [False, True])
@pytest.mark.parametrize("L", [6, 10])
def test_ipe_feature_and_cone_parameters(A, L, contracted):
    """ipe_feature_kernel (64-sample tiles) and cone_parameters_kernel on rows of 1, 7 and 128 frusta; N S on both sides of a tile; at
    L = 10 one call each with more tiles than the grid (1025 x 128 and 4097 x 128 frusta).  dn = max(|D|, 16) as a device scalar."""
    worst = {"mu_t": 0.0}
    for N, S in IPE_SHAPES + (((GRID_TILES * 64 // 128 + 1, 128),) if L == 10 else ()):
        rays, z = _ipe_inputs(N, S, contracted)
        dn = E.ipe_dn(rays)
        feat, mu, mu_t = A.ops.ipe_feature(z.cuda(), rays.cuda(), L, RADIUS, torch.tensor([dn], dtype=torch.float32).cuda(), contract=contracted)
        assert feat.shape == (N, S, 6 * L) and mu.shape == (N, S, 3)
        mode = "metric" if contracted else "plain"
        if contracted and N:
            assert E.sphere_gap(z, rays) >= E.SPHERE_GAP                          # every frustum mean: nothing is left out
        E.merge(worst, E.compare(E.ipe(z, rays, L, R2, dn, mode), {"pe": feat, "raw": mu}))
        cp = A.ops.cone_parameters(z.cuda(), RADIUS)
        E.merge(worst, E.compare(E.cone_parameters(z, R2), dict(zip(("mu_t", "var_t", "var_r"), cp))), "cone ")
        worst["mu_t"] += _bit_differences(mu_t, cp[0])                             # the encoder's third output is cone_moments' mu_t
    if L == 10 and not contracted:
        rays, z = _ipe_inputs(GRID_TILES * 256 // 128 + 1, 128, False)
        E.merge(worst, E.compare(E.cone_parameters(z, R2), dict(zip(("mu_t", "var_t", "var_r"), A.ops.cone_parameters(z.cuda(), RADIUS)))), "cone ")
    _emit("encoding ipe_feature L=%d contract=%d" % (L, contracted), worst, exact=("mu_t",))


def _table_columns():
    """element e of a 64-byte row = [lane half 0: K groups 0, 1 | lane half 1: K groups 0, 1] (8 bf16 each) -> reference column of
    [d | PE_4(d)] or -1 (include/nerf_amd.h nerf_amd_direction_table; the slot map of mlp_layout.h)"""
    return [R.pe_slot_column(e % 16, e // 16, 4) for e in range(32)]


def test_dirs_norm_and_direction_table(A):
    worst = {"pad": 0.0}
    cols = _table_columns()
    used = [e for e, c in enumerate(cols) if c >= 0]
    assert sorted(cols[e] for e in used) == list(range(27))
    for N in (1, 1023, 1024, 1025):
        rays = E.ray_batch(N, N)
        E.merge(worst, E.compare(E.dirs_norm(rays), {"dn": A.ops.dirs_norm(rays.cuda())}))
        table = A.ops.direction_table(rays.cuda()).float().cpu()
        assert table.shape == (N, 32)
        row = torch.zeros(N, 27)
        row[:, [cols[e] for e in used]] = table[:, used]
        worst["pad"] += float((table[:, [e for e, c in enumerate(cols) if c < 0]] != 0).sum())
        E.merge(worst, E.compare(E.direction_table(rays), {"dir-raw": row[:, :3], "dir-pe": row[:, 3:]}), "table ")
    _emit("encoding dirs_norm direction_table", worst, exact=("pad",))


# ------------------------------------------------------------------------------------------------ 2: the fused kernels
def _philox_u(seed, N, S):
    return O.philox_uniforms(seed, N, 0, S, 1)[0]


def _descriptor(A, src, contracted, keep, ipe=False, in_kernel_draw=False):
    """src (encoding_ref.make_source) -> nerf_amd_samples; `keep` holds the device tensors alive"""
    dev = {k: v.cuda() for k, v in src.items() if isinstance(v, torch.Tensor)}
    keep.append(dev)
    if src["mode"] == 0:
        s = A.Samples()
        s.mode, s.M, s.pts, s.pts_stride, s.contract = 0, src["pts"].shape[0], dev["pts"].data_ptr(), src["pts"].shape[1], int(contracted)
        return s
    S = src["S"]
    if src["mode"] == 1:
        if "z" in src:
            extra = {}
            if ipe:
                dn = torch.tensor([E.ipe_dn(src["rays"])], dtype=torch.float32).cuda()
                keep.append(dn)
                extra = dict(ipe_radius=RADIUS, ipe_dir_norm=dn)
            s = A.ops.samples_rays(dev["rays"], S, z=dev["z"], contract=contracted, **extra)
            assert s.z_stride == S + 3
            return s
        if in_kernel_draw:
            return A.ops.samples_rays(dev["rays"], S, z_base=dev["z_base"], z_jitter=src["z_jitter"], contract=contracted, seed=src["seed"])
        return A.ops.samples_rays(dev["rays"], S, z_base=dev["z_base"], u=dev["u"], z_jitter=src["z_jitter"], contract=contracted)
    s = A.Samples()
    s.mode, s.S, s.M, s.H, s.W, s.fx, s.fy, s.contract = 2, S, src["N"] * S, src["H"], src["W"], src["fx"], src["fy"], int(contracted)
    s.pose = (ctypes.c_float * 12)(*src["pose"])
    s.z_base, s.u, s.z_jitter, s.z_stride = dev["z_base"].data_ptr(), dev["u"].data_ptr(), src["z_jitter"], S
    return s


def _train(A, net, prec, s, M):
    fn = A.ops.proposal_forward_train_samples if net.name == "prop" else A.ops.mip_forward_train_samples
    return fn(net.packed(A, prec), TL._code(A, prec), s, (M,), "cuda")


def _infer(A, net, prec, s, M):
    fn = A.ops.proposal_forward_samples if net.name == "prop" else A.ops.mip_forward_samples
    return fn(net.packed(A, prec), TL._code(A, prec), s, (M,), "cuda")


def _slot(A, net, prec, M, dump):
    """the encoding slot -> ({output: rows in the reference's column order}, padding features that are not zero, the raw slot rows)"""
    enc = A.ops.train_dump_rows(dump, net.id, TL._code(A, prec), M, F.ENC_SLOT[net.name], F.ENC_WIDTH[net.name])
    ex, pad = R.slot_to_reference(enc[:, :64], 10)
    bad = float((pad != 0).sum())
    ed = None
    if net.name == "mip":
        ed, pad = R.slot_to_reference(enc[:, 64:96], 4)
        bad += float((pad != 0).sum())
    return E.slot_outputs(ex.float().cpu(), None if ed is None else ed.float().cpu()), bad, enc


def _sample_counts(A, prec):
    return (F.TILE[prec] - 1, F.TILE[prec] + 1, 3 * A.n_cu * F.TILE[prec] + 77)


@pytest.mark.parametrize("kind", E.SOURCES)
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_encoding_slot_against_the_fp64_specification(A, name, prec, kind):
    """Part 2.  For the explicit-z source of the fine network also the integrated PE, plain (contract = 0) and metric (contract = 1)."""
    net = TL._net(A, name, "he")
    worst = {"padding": 0.0}
    exact = ["padding"]
    t0 = time.time()
    for contracted in (False, True):
        for M in _sample_counts(A, prec):
            src = E.make_source(kind, name, M, contracted, philox_u=_philox_u)
            for ipe in ((False, True) if (kind == "z" and name == "mip") else (False,)):
                keep = []
                out, dump = _train(A, net, prec, _descriptor(A, src, contracted, keep, ipe=ipe), M)
                got, bad, enc = _slot(A, net, prec, M, dump)
                assert bool(torch.isfinite(out).all())
                bounds, gap = E.fused(src, name, prec, contracted, ipe_args=(R2, E.ipe_dn(src["rays"])) if ipe else None)
                if contracted:
                    assert gap >= E.SPHERE_GAP, "a sample within %.1e of the unit sphere" % gap          # all of them: no sample is left out
                E.merge(worst, E.compare(bounds, got), "ipe-" if ipe else "")
                if not ipe:
                    own = E.own_inputs(got, prec)
                    E.merge(worst, E.compare(own, {"pos-pe|raw": got["pos-pe"], "dir-pe|raw": got.get("dir-pe")}))
                worst["padding"] += bad
                if kind.startswith("pts") and not contracted and prec == "fp32":                        # the position is an input: its bits
                    worst["raw-bits"] = worst.get("raw-bits", 0.0) + _bit_differences(got["pos-raw"], src["pts"][:, :3])
                    exact.append("raw-bits")
                if kind == "philox" and not ipe:
                    u_dev = A.ops.philox_stream((src["u"].shape[0], src["S"]), src["seed"], strat=True)
                    worst["philox-stream"] = worst.get("philox-stream", 0.0) + _bit_differences(u_dev.cpu(), src["u"])
                    out2, dump2 = _train(A, net, prec, _descriptor(A, src, contracted, keep, in_kernel_draw=True), M)
                    enc2 = A.ops.train_dump_rows(dump2, net.id, TL._code(A, prec), M, F.ENC_SLOT[name], F.ENC_WIDTH[name])
                    worst["in-kernel-draw"] = worst.get("in-kernel-draw", 0.0) + _bit_differences(enc2, enc) + _bit_differences(out2, out)
                    exact += ["philox-stream", "in-kernel-draw"]
                    del dump2
                del dump
    torch.cuda.synchronize()
    print("encoding slot %s %s %s: %.1f s" % (name, prec, kind, time.time() - t0))
    _emit("encoding slot %s %s %s" % (name, prec, kind), worst, exact=tuple(exact))


# ------------------------------------------------------------------------------------------------ 3: render == training forward
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["prop", "mip"])
def test_inference_entry_points_equal_the_training_forward_on_ray_descriptors(A, name, prec):
    """the ray sources at the two small sample counts, contraction off and on, and the in-kernel Philox draw"""
    net = TL._net(A, name, "he")
    worst = {}
    for kind in ("z", "u", "philox", "cam"):
        worst[kind] = 0.0
        for contracted in (False, True):
            for M in _sample_counts(A, prec)[:2]:
                src = E.make_source(kind, name, M, contracted, philox_u=_philox_u)
                for draw in ((False, True) if kind == "philox" else (False,)):
                    keep = []
                    out, dump = _train(A, net, prec, _descriptor(A, src, contracted, keep, in_kernel_draw=draw), M)
                    del dump
                    worst[kind] += _bit_differences(_infer(A, net, prec, _descriptor(A, src, contracted, keep, in_kernel_draw=draw), M), out)
    _emit("encoding inference == training %s %s" % (name, prec), worst, exact=tuple(worst))
