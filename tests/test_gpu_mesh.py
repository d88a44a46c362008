"""Iso-surface extraction on the GPU (nerf_amd_mesh_count / nerf_amd_mesh_emit, nerf_amd.mesh): the kernels against the fp64, table-free
specification of tests/mesh_ref.py -- counts and faces EXACTLY (order, diagonal, winding), positions and normals within the bounds derived
there from the shipped arithmetic (error / bound <= 1 through conftest.gate, which records every figure) --, the topology of closed and
open surfaces, ties and non-finite entries, determinism whatever the buffers held, the guarded stores, and the network-facing layer:
density_grid against the networks' own forwards bit for bit, extract_mesh, vertex colours and render_only --mesh."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_ref as R
from conftest import gate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import nerf_amd
    nerf_amd.set_precision("fp32")
    yield
    nerf_amd.set_precision("fp32")


def _mt(field, iso, **kw):
    from nerf_amd import mesh
    out = mesh.marching_tetrahedra(torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32)).cuda(), iso, **kw)
    assert out["vertices"].dtype == torch.float32 and out["faces"].dtype == torch.int32 and all(t.is_cuda for t in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(name, got, want, normals=True):
    bad, pos, nrm = R.compare(got, want, normals=normals)
    assert bad == [], bad
    gate("mesh %s: position error / bound" % name, pos, 1.0)
    if normals:
        gate("mesh %s: normal error / bound" % name, nrm, 1.0)


_SPECS = {}


def _spec(name, make, iso, **kw):
    """one specification per (field, iso, placement), shared among the tests"""
    if name not in _SPECS:
        f = make()
        _SPECS[name] = (f, R.spec(f, iso, **kw))
    return _SPECS[name]


# ------------------------------------------------------------------------------------------------ 1. all 256 corner-sign patterns
def test_all_256_corner_sign_patterns():
    rng = np.random.default_rng(256)
    worst = 0.0
    n_faces = 0
    for pattern in range(256):
        mag = rng.uniform(0.1, 1.0, size=8)
        sign = np.where((pattern >> np.arange(8)) & 1, 1.0, -1.0)
        f = (mag * sign).astype(np.float32).reshape(2, 2, 2)                       # corner c = dx + 2 dy + 4 dz at [dz, dy, dx]
        want = R.spec(f, 0.0)
        got = _mt(f, 0.0)
        bad, pos, nrm = R.compare(got, want)
        assert bad == [], (pattern, bad)
        assert (len(want["faces"]) == 0) == (pattern in (0, 255))
        worst = max(worst, pos, nrm)
        n_faces += len(want["faces"])
    assert n_faces > 1000
    gate("mesh 256 patterns: worst error / bound", worst, 1.0)


# ------------------------------------------------------------------------------------------------ 2. noise fields
@pytest.mark.parametrize("iso", (0.0, 0.25))
@pytest.mark.parametrize("shape", ((5, 7, 9), (17, 33, 65)), ids=lambda s: "x".join(map(str, s)))
def test_noise_fields(shape, iso):
    f, want = _spec("noise%s@%g" % (shape, iso), lambda: R.noise_field(shape), iso)
    got = _mt(f, iso)
    assert len(got["vertices"]) == len(want["vertices"]) > 0 and len(got["faces"]) == len(want["faces"]) > 0
    if shape == (17, 33, 65):
        assert f.size > 100 * 256 and all(n % 256 and n % 64 for n in shape)          # many tiles of 256 points (the tile scan's own steps:
        #                                                                               test_lattice_of_more_than_one_scan_step); no dimension a multiple of a tile
    assert np.array_equal(got["faces"], want["faces"])
    _check("noise %s iso %g" % (shape, iso), got, want)


def test_lattice_of_more_than_one_scan_step():
    """4 456 tiles of 256 points, each with counts: the tile scan (4 tiles per thread, 1 024 per group, 4 096 per step) runs all four
    waves and all four groups of a full step, carries into a second step that it loaded one step ahead, and ends in a partial group.
    Every vertex and face id depends on those prefixes: faces are compared exactly."""
    from nerf_amd import _lib
    f, want = _spec("gyroid", R.gyroid_field, 0.0)
    assert (f.size + 255) // 256 > _lib.MESH_SCAN_STEP_TILES >= 4096
    assert all(n % 256 and n % 1024 for n in f.shape) and ((f.size + 255) // 256) % 1024 not in (0, 1023)
    got = _mt(f, 0.0)
    assert len(got["vertices"]) == len(want["vertices"]) > 500000 and len(got["faces"]) == len(want["faces"]) > 1000000
    assert int(got["faces"].min()) == 0 and int(got["faces"].max()) == len(got["vertices"]) - 1
    assert np.array_equal(got["faces"], want["faces"])
    _check("gyroid (97, 105, 112)", got, want)
    dev = torch.from_numpy(f).cuda()
    runs = [_raw(dev, 0.0, fill) for fill in (0x00, 0xFF)]
    assert runs[0][0] == runs[1][0] == (len(want["vertices"]), len(want["faces"]))
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert np.array_equal(runs[0][3].cpu().numpy(), want["faces"])


# ------------------------------------------------------------------------------------------------ 3. closed surfaces
@pytest.mark.parametrize("name", sorted(R.CLOSED))
def test_closed_surfaces(name):
    make, chi = R.CLOSED[name]
    f, want = _spec(name, make, 0.0)
    assert float(want["normal_bound"].max()) < R.VACUOUS, "the normal check must not be empty on this field"
    got = _mt(f, 0.0)
    _check(name, got, want)
    closed, v_used, _, _ = R.edge_census(got["faces"])
    assert closed and v_used == len(got["vertices"])
    assert R.euler_characteristic(got["faces"]) == chi
    vol, vol_want = R.signed_volume(got["vertices"], got["faces"]), R.signed_volume(want["vertices"], want["faces"])
    assert vol > 0.0
    # volume = sum of p0 . (p1 x p2) / 6: moving corner i by e changes a term by at most |e| |p_j| |p_k|; 1-norms for the 2-norms, face by face
    v = np.abs(want["vertices"])[want["faces"]]                                  # (F, 3 corners, 3 axes)
    b = want["pos_bound"][want["faces"]]
    size = v.sum(-1).max(1)
    slack = float((b.sum(-1).sum(1) * size * size).sum() / 6.0) * 1.001 + 1e-9 * abs(vol_want)     # (+ the fp64 sums' own rounding)
    gate("mesh %s: |volume - spec| / rounding slack" % name, abs(vol - vol_want), slack)


# ------------------------------------------------------------------------------------------------ 4. ties and specials
def test_ties_stay_closed():
    f, want = _spec("ties", R.integer_ball_field, 0.0)
    assert int((f == 0).sum()) >= 20
    got = _mt(f, 0.0)
    _check("integer ball", got, want)
    assert R.edge_census(got["faces"])[0] and R.euler_characteristic(got["faces"]) == 2


def test_nan_and_infinite_entries():
    f, want = _spec("specials", R.specials_field, 0.0)
    assert np.isnan(f).sum() == 1 and np.isposinf(f).sum() == 1 and np.isneginf(f).sum() == 1
    got = _mt(f, 0.0)
    assert np.isfinite(got["vertices"]).all() and np.isfinite(got["normals"]).all()
    _check("nan / inf entries", got, want)                                       # (faces and counts exactly; normals where the bound is finite)


# ------------------------------------------------------------------------------------------------ 5. open surface
def test_open_surface_boundary_is_on_the_lattice_faces():
    shape = (5, 7, 9)
    f, want = _spec("noise%s@%g" % (shape, 0.0), lambda: R.noise_field(shape), 0.0)
    got = _mt(f, 0.0)
    edges = R.boundary_edges(got["faces"])
    assert len(edges) > 0
    hi = np.asarray((shape[2] - 1, shape[1] - 1, shape[0] - 1), dtype=np.float32)
    on = lambda v: (got["vertices"][v] == 0.0) | (got["vertices"][v] == hi)      # exact: a + 0 t on the axis across the face
    assert (on(edges[:, 0]) & on(edges[:, 1])).any(1).all()


# ------------------------------------------------------------------------------------------------ 6. spacing and origin
def test_spacing_and_origin():
    origin, spacing = (100.0, -50.0, 7.0), (0.5, 2.0, 1.25)
    f, want = _spec("sphere far", R.sphere_field, 0.0, origin=origin, spacing=spacing)
    got = _mt(f, 0.0, origin=origin, spacing=spacing)
    _check("sphere, anisotropic spacing, far origin", got, want)
    plain = _mt(f, 0.0)
    assert np.array_equal(plain["faces"], got["faces"])
    assert not np.array_equal(plain["vertices"], got["vertices"])
    f2, want2 = _spec("noise far", lambda: R.noise_field((6, 5, 7), seed=3), 0.1, origin=(-3.0, 1e4, 0.25), spacing=(3.0, 0.01, 1.0))
    _check("noise, spacing (3, 0.01, 1), origin (-3, 1e4, 0.25)", _mt(f2, 0.1, origin=(-3.0, 1e4, 0.25), spacing=(3.0, 0.01, 1.0)), want2)
    no_normals = _mt(f, 0.0, normals=False)
    assert set(no_normals) == {"vertices", "faces"} and np.array_equal(no_normals["vertices"], plain["vertices"])


# ------------------------------------------------------------------------------------------------ 7. determinism and empty cases
def _raw(field, iso, fill, v_cap=None, f_cap=None, pad=0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """the two C entry points on buffers whose every byte was `fill` -> (counts, vertices, normals, faces) with `pad` sentinel rows kept"""
    from nerf_amd import _lib
    nz, ny, nx = field.shape
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    new = lambda n, dtype: torch.empty((max(n, 1) * torch.empty((), dtype=dtype).element_size(),), dtype=torch.uint8, device="cuda").fill_(fill).view(dtype)
    n_ws = _lib.lib.nerf_amd_mesh_workspace_bytes(nx, ny, nz)
    assert n_ws >= 5 * field.numel()
    ws, counts = new(n_ws, torch.uint8), new(2, torch.int64)
    _lib.check(_lib.lib.nerf_amd_mesh_count(p(field), nx, ny, nz, iso, p(counts), p(ws), st), "nerf_amd_mesh_count")
    V, F = (int(c) for c in counts.tolist())
    v_cap, f_cap = V if v_cap is None else v_cap, F if f_cap is None else f_cap
    vertices, normals, faces = new(3 * (v_cap + pad), torch.float32), new(3 * (v_cap + pad), torch.float32), new(3 * (f_cap + pad), torch.int32)
    o3, s3 = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing)
    _lib.check(_lib.lib.nerf_amd_mesh_emit(p(field), nx, ny, nz, iso, o3, s3, p(ws), v_cap, f_cap, p(vertices), p(normals), p(faces), st), "nerf_amd_mesh_emit")
    torch.cuda.synchronize()
    return (V, F), vertices.view(-1, 3), normals.view(-1, 3), faces.view(-1, 3)


def test_bits_do_not_depend_on_what_the_buffers_held():
    f = torch.from_numpy(R.noise_field((17, 33, 65))).cuda()
    runs = [_raw(f, 0.25, fill) for fill in (0x00, 0xFF, 0xFF)]
    want = _SPECS.get("noise%s@%g" % ((17, 33, 65), 0.25))
    if want is not None:
        assert runs[0][0] == (len(want[1]["vertices"]), len(want[1]["faces"]))
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        for a, b in zip(runs[0][1:], other[1:]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    from nerf_amd import mesh
    again = mesh.marching_tetrahedra(f, 0.25)
    assert torch.equal(again["vertices"].view(torch.int32), runs[0][1].view(torch.int32)) and torch.equal(again["faces"], runs[0][3])
    assert torch.equal(again["normals"].view(torch.int32), runs[0][2].view(torch.int32))


def test_empty_surface_and_sliver():
    f = R.noise_field((5, 7, 9))
    for iso in (float(f.max()) + 1.0, float(f.min())):                           # nothing inside; everything inside (f >= iso)
        got = _mt(f, iso)
        assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["normals"].shape == (0, 3)
    sliver = R.noise_field((301, 2, 2), seed=5)                                  # 2 x 2 x N: every point on the boundary
    want = R.spec(sliver, 0.0)
    _check("2 x 2 x 301 sliver", _mt(sliver, 0.0), want)
    _check("301 x 2 x 2 sliver", _mt(np.ascontiguousarray(sliver.reshape(2, 2, 301)), 0.0), R.spec(sliver.reshape(2, 2, 301), 0.0))


# ------------------------------------------------------------------------------------------------ 8. guarded stores
def test_stores_are_guarded_by_the_capacities():
    """capacities below the counts: the first entries are what the full run stores, and not one byte beyond the capacity is touched
    (the stores are guarded; nothing here runs out of bounds)"""
    f = torch.from_numpy(R.noise_field((9, 10, 11))).cuda()
    (V, F), vertices, normals, faces = _raw(f, 0.0, 0xA5)
    assert V > 300 and F > 500
    pad = 64
    for v_cap, f_cap in ((V // 2, F // 3), (0, F), (V, 0), (1, 1)):
        counts, v2, n2, f2 = _raw(f, 0.0, 0xA5, v_cap=v_cap, f_cap=f_cap, pad=pad)
        assert counts == (V, F)
        assert torch.equal(v2[:v_cap].view(torch.int32), vertices[:v_cap].view(torch.int32))
        assert torch.equal(n2[:v_cap].view(torch.int32), normals[:v_cap].view(torch.int32))
        assert torch.equal(f2[:f_cap], faces[:f_cap])
        sentinel = torch.full((1,), 0xA5, dtype=torch.uint8, device="cuda")
        for buf, cap in ((v2, v_cap), (n2, v_cap), (f2, f_cap)):
            tail = buf.reshape(-1)[3 * cap:].view(torch.uint8)
            assert tail.numel() >= 12 * pad and bool((tail == sentinel).all())


def test_entry_points_refuse_bad_arguments():
    from nerf_amd import _lib
    lib = _lib.lib
    f = torch.zeros((3, 4, 5), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws = torch.empty((int(lib.nerf_amd_mesh_workspace_bytes(5, 4, 3)),), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    out = torch.zeros((64,), dtype=torch.float32, device="cuda")
    o3, s3 = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1)
    EINVAL = lib.nerf_amd_mesh_count(None, 5, 4, 3, 0.0, p(counts), p(ws), None)
    assert EINVAL != 0
    assert lib.nerf_amd_mesh_workspace_bytes(1, 4, 3) == 0 and lib.nerf_amd_mesh_workspace_bytes(2048, 2048, 512) == 0
    assert lib.nerf_amd_mesh_workspace_bytes(2047, 2048, 512) > 0
    bad_count = [(p(f), 1, 4, 3, 0.0, p(counts), p(ws)), (p(f), 5, 4, 3, float("nan"), p(counts), p(ws)), (p(f), 5, 4, 3, float("inf"), p(counts), p(ws)),
                 (p(f), 5, 4, 3, 0.0, None, p(ws)), (p(f), 5, 4, 3, 0.0, p(counts), None), (p(f), 2048, 2048, 512, 0.0, p(counts), p(ws))]
    for args in bad_count:
        assert lib.nerf_amd_mesh_count(*args, None) == EINVAL, args
    nan3, zero3, inf3 = (ctypes.c_float * 3)(0, float("nan"), 0), (ctypes.c_float * 3)(1, 0, 1), (ctypes.c_float * 3)(1, float("inf"), 1)
    good = [p(f), 5, 4, 3, 0.0, o3, s3, p(ws), 4, 4, p(out), p(out), p(out)]
    for at, value in ((0, None), (1, 1), (4, float("nan")), (5, None), (5, nan3), (6, None), (6, zero3), (6, inf3), (7, None), (8, -1), (9, -1), (8, 2 ** 31),
                      (9, 2 ** 31 // 3 + 1), (10, None), (12, None)):
        args = list(good)
        args[at] = value
        assert lib.nerf_amd_mesh_emit(*args, None) == EINVAL, (at, value)
    torch.cuda.synchronize()
    assert int(counts.sum()) == 0 and float(out.abs().sum()) == 0.0                # refused before any launch


def test_refused_on_a_capturing_stream():
    from nerf_amd import mesh
    f = torch.from_numpy(R.sphere_field()).cuda()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    caught, keep = None, torch.zeros(8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):                             # refused on the host before any launch: the graph holds the one add
        keep.add_(1.0)
        try:
            mesh.marching_tetrahedra(f, 0.0)
        except RuntimeError as e:
            caught = str(e)
    torch.cuda.synchronize()
    assert caught is not None and "captur" in caught
    assert mesh.marching_tetrahedra(f, 0.0)["faces"].shape[0] == 1212      # and the same call outside a capture still runs


# ------------------------------------------------------------------------------------------------ 9. networks
def _net(kind):
    from nerf_amd import synthetic_weights as SW
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.ref_model import RefNeRF
    if kind == "proposal":
        net = ProposalNetwork(10, 256)
        net.load_state_dict(SW.proposal_state("he"))
    elif kind == "mip":
        net = MipNeRF(10, 4, 256)
        net.load_state_dict(SW.mip_state("he"))
    else:
        net = RefNeRF(10, 4)
        net.load_state_dict(SW.ref_state("he"))
    return net.cuda().eval()


RES = (9, 10, 11)                                        # (nx, ny, nz)
BOX = ((-1.2, -0.9, -1.1), (1.1, 1.3, 0.8))


def _lattice_points():
    lo, hi = np.asarray(BOX[0]), np.asarray(BOX[1])
    axes = [(lo[a] + (hi[a] - lo[a]) * np.arange(m, dtype=np.float64) / (m - 1)).astype(np.float32) for a, m in enumerate(RES)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.from_numpy(np.stack((x, y, z), -1).reshape(-1, 3)).cuda()


def _own_forward(net, kind, pos, dirs, contract):
    with torch.no_grad():
        if kind == "proposal":
            return net(pos.view(-1, 1, 3), contract=contract).reshape(-1), None
        out = net(torch.cat((pos, dirs), -1).view(-1, 1, 6), contract=contract)
        rgbo = (out[0] if kind == "ref" else out).reshape(-1, 4)
        return rgbo[:, 3], rgbo[:, :3]


@pytest.mark.parametrize("contract", (False, True), ids=("plain", "contract"))
@pytest.mark.parametrize("kind", ("proposal", "mip", "ref"))
def test_density_grid_and_extract_mesh_on_the_networks(kind, contract):
    from nerf_amd import mesh
    net = _net(kind)
    pos = _lattice_points()
    dirs = torch.tensor((0.0, 0.0, -1.0), device="cuda").expand(pos.shape[0], 3)
    sigma, _ = _own_forward(net, kind, pos, dirs, contract)
    want_raw = sigma.view(RES[2], RES[1], RES[0])
    want = torch.nn.functional.softplus(want_raw + 0.5) if kind == "ref" else torch.relu(want_raw)
    for chunk in (1 << 22, 97, 1000):
        field, origin, spacing = mesh.density_grid(net, BOX, RES, contract=contract, chunk_points=chunk)
        assert field.shape == (RES[2], RES[1], RES[0]) and field.dtype == torch.float32 and field.is_contiguous()
        assert torch.equal(field, want), (kind, contract, chunk)
    raw, _, _ = mesh.density_grid(net, BOX, RES, contract=contract, activation="raw", chunk_points=97)
    assert torch.equal(raw, want_raw)
    assert origin == tuple(float(np.float32(v)) for v in BOX[0])
    assert spacing == tuple(float(np.float32((BOX[1][a] - BOX[0][a]) / (RES[a] - 1))) for a in range(3))
    cube, _, _ = mesh.density_grid(net, BOX, 4, contract=contract)
    assert cube.shape == (4, 4, 4)
    # extract_mesh = density_grid + marching_tetrahedra, at the median so that the surface is there (of the raw field: after a ReLU the
    # median may be the minimum, 0, and f >= 0 everywhere is an empty surface)
    field = raw
    iso = float(field.median())
    a = mesh.marching_tetrahedra(field, iso, origin=origin, spacing=spacing)
    assert a["vertices"].shape[0] > 0 and a["faces"].shape[0] > 0
    b = mesh.extract_mesh(net, BOX, RES, iso, contract=contract, colors=kind != "proposal", activation="raw", chunk_points=1000)
    for k in ("vertices", "faces", "normals"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    _check("%s field%s" % (kind, " contracted" if contract else ""), {k: v.cpu().numpy() for k, v in a.items()},
           R.spec(field.cpu().numpy(), iso, origin=origin, spacing=spacing))
    # ... and with the default "render" activation, at a level between the field's extremes (a ReLU field's median can be its minimum)
    if kind != "proposal":
        lo, hi = float(want.min()), float(want.max())
        assert hi > lo
        level = 0.5 * (lo + hi)
        c = mesh.marching_tetrahedra(want.contiguous(), level, origin=origin, spacing=spacing)
        d = mesh.extract_mesh(net, BOX, RES, level, contract=contract, chunk_points=97)
        assert c["faces"].shape[0] > 0 and set(d) == {"vertices", "faces", "normals"}
        for k in ("vertices", "faces", "normals"):
            assert torch.equal(c[k].view(torch.int32), d[k].view(torch.int32)), k
    if kind == "proposal":
        assert "colors" not in b
        return
    view = torch.where((b["normals"] == 0).all(-1, keepdim=True), torch.tensor((0.0, 0.0, -1.0), device="cuda"), -b["normals"])
    _, rgb = _own_forward(net, kind, b["vertices"], view, contract)
    assert b["colors"].shape == b["vertices"].shape and b["colors"].dtype == torch.float32 and torch.equal(b["colors"], rgb.float())


# ------------------------------------------------------------------------------------------------ 10. render_only --mesh
def test_render_only_writes_the_mesh(tmp_path, capsys):
    import json
    from PIL import Image
    import nerf_amd
    from nerf_amd import mesh, procedures, synthetic_weights as SW
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    from nerf_amd.nerf_helper import saveModel
    from nerf_amd.utils import pose_spherical
    nerf_amd.set_precision(None)
    root = str(tmp_path)
    scene = os.path.join(root, "data", "toy")
    os.makedirs(os.path.join(scene, "test"))
    rng = np.random.default_rng(4)
    Image.fromarray(rng.integers(0, 255, size=(24, 24, 3), dtype=np.uint8)).save(os.path.join(scene, "test", "r_0.png"))
    frames = [{"file_path": "./test/r_0", "transform_matrix": pose_spherical(0.0, -30.0, 4.0).tolist()}]
    json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(os.path.join(scene, "transforms_test.json"), "w"))
    prop, mip = ProposalNetwork(10, 256), MipNeRF(10, 4, 256)
    prop.load_state_dict(SW.proposal_state("he"))
    mip.load_state_dict(SW.mip_state("he"))
    prop, mip = prop.cuda().eval(), mip.cuda().eval()
    os.makedirs(os.path.join(root, "model"))
    saveModel(mip, os.path.join(root, "model", "toy_mip.pth"))
    saveModel(prop, os.path.join(root, "model", "toy_prop.pth"))
    with torch.no_grad():
        field, _, _ = mesh.density_grid(mip, ((-1.5,) * 3, (1.5,) * 3), 12)
    iso = 0.5 * (float(field.min()) + float(field.max()))                       # between the extremes: the surface is there
    want = mesh.extract_mesh(mip, ((-1.5,) * 3, (1.5,) * 3), 12, iso, colors=True)
    assert want["faces"].shape[0] > 0
    ply = os.path.join(root, "toy.ply")
    base = ["--name", "toy", "--dataset_name", "toy", "--img_scale", "1.0", "--opt_mode", "none", "-e", "-w"]
    texts = {}
    for flag in (False, True):
        extra = ["--mesh", ply, "--mesh_res", "12", "--mesh_iso", repr(iso)] if flag else []
        torch.manual_seed(3)                                                     # (the renderer draws its jitter from torch's generator)
        procedures.render_only(procedures.get_parser().parse_args(base + extra), os.path.join(root, "model") + "/", "O1",
                               dataset_root=os.path.join(root, "data") + "/", output_root=os.path.join(root, "out_%d" % flag) + "/")
        texts[flag] = capsys.readouterr().out.splitlines()
        assert os.path.exists(ply) == flag
    assert texts[True][:-1] == texts[False] and texts[True][-1].startswith("Mesh: %d vertices, %d faces" % (want["vertices"].shape[0], want["faces"].shape[0]))
    assert open(os.path.join(root, "out_0", "given", "result_000.png"), "rb").read() == open(os.path.join(root, "out_1", "given", "result_000.png"), "rb").read()
    props, faces = R.read_ply(ply)
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert len(props["x"]) == want["vertices"].shape[0] and faces.shape == tuple(want["faces"].shape)
    assert np.array_equal(faces, want["faces"].cpu().numpy())
    assert np.array_equal(np.stack([props[k] for k in "xyz"], 1), want["vertices"].cpu().numpy())
