"""Iso-surface extraction, host side: the fp64 specification's own properties on the anchor fields (closed, oriented, Euler characteristic,
volume), its bounds against the shipped arithmetic restated in numpy float32, the planted faults that the comparator must catch, the PLY
writer against a reader that lives with the tests, and every ValueError of nerf_amd.mesh -- all raised before a device is needed."""
import numpy as np
import pytest
import torch

import mesh_ref as R
from nerf_amd import mesh

ORIGIN, SPACING = (100.0, -50.0, 7.0), (0.5, 2.0, 1.25)


@pytest.fixture(scope="module")
def specs():
    return {name: R.spec(make(), 0.0) for name, (make, _) in R.CLOSED.items()}


# ------------------------------------------------------------------------------------------------ the specification on the anchors
@pytest.mark.parametrize("name,V,E,F,chi,volume", [("sphere", 608, 1818, 1212, 2, 140.3330), ("torus", 1198, 3594, 2396, 0, 188.0198),
                                                   ("two_spheres", 490, 1458, 972, 4, None)])
def test_anchor_fields(specs, name, V, E, F, chi, volume):
    sp = specs[name]
    closed, v_used, e, f = R.edge_census(sp["faces"])
    assert closed, "every undirected edge in exactly two faces, once in each direction"
    assert (len(sp["vertices"]), v_used, e, f) == (V, V, E, F)
    assert R.euler_characteristic(sp["faces"]) == chi == R.CLOSED[name][1]
    vol = R.signed_volume(sp["vertices"], sp["faces"])
    assert vol > 0.0
    if volume is not None:
        assert abs(vol - volume) < 1e-4
    assert float(sp["normal_bound"].max()) < R.VACUOUS and float(sp["pos_bound"].max()) < 1e-5


def test_noise_anchor_counts():
    sp = R.spec(R.noise_field((17, 33, 65)), 0.0)
    assert 1.1e5 < len(sp["vertices"]) < 1.3e5 and 2.3e5 < len(sp["faces"]) < 2.7e5
    assert sp["faces"].min() == 0 and sp["faces"].max() == len(sp["vertices"]) - 1


def test_spec_geometry(specs):
    """vertices lie on their edges, measured from the owner; normals are unit, point outwards (from high values to low) and agree with
    the winding; the vertex list is in ascending (point, slot) order"""
    f = R.sphere_field()
    sp = R.spec(f, 0.0, ORIGIN, SPACING)
    a, d, t = sp["owner"], sp["direction"], sp["t"]
    assert ((t >= 0.0) & (t <= 1.0)).all()
    assert np.allclose(sp["vertices"], np.asarray(ORIGIN) + np.asarray(SPACING) * (a + t[:, None] * d), rtol=0, atol=1e-12)
    nz, ny, nx = f.shape
    key = ((a[:, 2] * ny + a[:, 1]) * nx + a[:, 0]) * 7 + (d[:, 0] + 2 * d[:, 1] + 4 * d[:, 2] - 1)
    assert (np.diff(key) > 0).all()
    # t is the crossing of the linear interpolant, from the owner
    fa = f[a[:, 2], a[:, 1], a[:, 0]].astype(np.float64)
    b = a + d
    fb = f[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64)
    assert np.allclose(fa + t * (fb - fa), 0.0, atol=1e-9)
    n = sp["normals"]
    assert np.allclose((n * n).sum(1), 1.0)
    centre = np.asarray(ORIGIN) + np.asarray(SPACING) * np.asarray((5.1, 5.4, 6.2))
    assert ((n * (sp["vertices"] - centre) / np.asarray(SPACING) ** 2).sum(1) > 0).all()      # outwards (the gradient of the quadric, axis by axis)
    v = sp["vertices"]
    p0, p1, p2 = (v[sp["faces"][:, q]] for q in range(3))
    face_n = np.cross(p1 - p0, p2 - p0)
    assert ((face_n * (n[sp["faces"][:, 0]] + n[sp["faces"][:, 1]] + n[sp["faces"][:, 2]])).sum(1) > 0).all()
    # spacing and origin change no face
    assert np.array_equal(sp["faces"], specs["sphere"]["faces"])


def test_ties_and_specials_in_the_spec():
    f = R.integer_ball_field()
    assert int((f == 0).sum()) >= 20
    sp = R.spec(f, 0.0)
    assert R.edge_census(sp["faces"])[0] and R.euler_characteristic(sp["faces"]) == 2
    sp = R.spec(R.specials_field(), 0.0)
    assert np.isfinite(sp["vertices"]).all() and np.isfinite(sp["normals"]).all() and len(sp["faces"]) > 0
    assert (sp["t"] == 0.5).any()


def test_open_surface_boundary_lies_on_the_lattice_faces():
    f = R.noise_field((5, 7, 9))
    sp = R.spec(f, 0.0)
    edges = R.boundary_edges(sp["faces"])
    assert len(edges) > 0
    hi = np.asarray((8, 6, 4), dtype=np.float64)
    on = lambda v: (sp["vertices"][v] == 0.0) | (sp["vertices"][v] == hi)
    assert (on(edges[:, 0]) & on(edges[:, 1])).any(1).all()


# ------------------------------------------------------------------------------------------------ the bounds against the shipped arithmetic
@pytest.mark.parametrize("case", ["sphere", "torus", "two_spheres", "noise", "noise_far", "ties", "specials"])
def test_bounds_cover_the_shipped_arithmetic(case):
    origin, spacing, iso = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0
    if case in R.CLOSED:
        f = R.CLOSED[case][0]()
    elif case == "noise":
        f, iso = R.noise_field((9, 10, 11)), 0.25
    elif case == "noise_far":
        f, origin, spacing = R.noise_field((9, 10, 11)), ORIGIN, SPACING
    elif case == "ties":
        f = R.integer_ball_field()
    else:
        f = R.specials_field()
    want = R.spec(f, iso, origin, spacing)
    bad, pos, nrm = R.compare(R.shipped_arithmetic(f, iso, origin, spacing), want)
    print("%s: worst position error / bound %.3f, worst normal error / bound %.3f" % (case, pos, nrm))
    assert bad == []
    assert 0.0 < pos <= 1.0 and nrm <= 1.0


# ------------------------------------------------------------------------------------------------ planted faults
@pytest.mark.parametrize("fault", R.FAULTS)
def test_comparator_catches_planted_fault(fault):
    """The clamp proper can never bind on a crossed edge -- iso lies between the two values and fp32 subtraction and division are monotone,
    so 0 <= t <= 1 already --: `no_clamp` drops the step the clamp is part of (clamp + the non-finite rule), which shows on the field
    with NaN and infinite entries."""
    assert len(R.FAULTS) >= 7
    f = R.specials_field() if fault == "no_clamp" else R.sphere_field()
    want = R.spec(f, 0.0, ORIGIN, SPACING)
    assert R.compare(want, want)[0] == []
    bad, _, _ = R.compare(R.spec(f, 0.0, ORIGIN, SPACING, fault=fault), want)
    assert bad, "the comparator let '%s' through" % fault


def test_comparator_catches_a_wrong_normal_and_a_wrong_count(specs):
    want = specs["sphere"]
    got = {k: want[k].copy() for k in ("vertices", "faces", "normals")}
    got["normals"][7] = -got["normals"][7]
    assert R.compare(got, want)[0]
    got = {"vertices": want["vertices"][:-1], "faces": want["faces"], "normals": want["normals"][:-1]}
    assert R.compare(got, want)[0]


# ------------------------------------------------------------------------------------------------ PLY
@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (True, True), (False, True)])
def test_ply_round_trip(tmp_path, specs, with_normals, with_colors):
    sp = specs["torus"]
    v, f, n = sp["vertices"].astype(np.float32), sp["faces"], sp["normals"].astype(np.float32)
    colors = np.random.default_rng(2).uniform(-0.2, 1.2, size=v.shape).astype(np.float32)
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(n) if with_normals else None, colors if with_colors else None)
    props, faces = R.read_ply(path)
    assert list(props) == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert np.array_equal(np.stack([props[k] for k in "xyz"], 1), v) and np.array_equal(faces, f)
    if with_normals:
        assert np.array_equal(np.stack([props[k] for k in ("nx", "ny", "nz")], 1), n)
    if with_colors:
        want = np.rint(np.clip(colors.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        assert np.array_equal(np.stack([props[k] for k in ("red", "green", "blue")], 1), want)
        assert want.min() == 0 and want.max() == 255


def test_write_ply_refuses_bad_shapes(tmp_path):
    v, f = np.zeros((4, 3), np.float32), np.zeros((2, 3), np.int32)
    for args in ((v[:, :2], f), (v, f[:, :2]), (v, f, v[:3]), (v, f, None, v[:3])):
        with pytest.raises(ValueError):
            mesh.write_ply(str(tmp_path / "bad.ply"), *args)


# ------------------------------------------------------------------------------------------------ every ValueError, ahead of any device
GOOD = torch.zeros((3, 4, 5), dtype=torch.float32)


@pytest.mark.parametrize("field,kw,what", [
    (np.zeros((3, 4, 5), np.float32), {}, "torch.Tensor"),
    (GOOD.double(), {}, "float32"),
    (GOOD[0], {}, "(nz, ny, nx)"),
    (GOOD[None], {}, "(nz, ny, nx)"),
    (GOOD.transpose(0, 2), {}, "contiguous"),
    (GOOD[:, :, :1].contiguous(), {}, "at least 2"),
    (GOOD, {"iso": float("nan")}, "iso"),
    (GOOD, {"iso": float("inf")}, "iso"),
    (GOOD, {"iso": 1e39}, "iso"),
    (GOOD, {"spacing": (1.0, 0.0, 1.0)}, "spacing"),
    (GOOD, {"spacing": (1.0, -1.0, 1.0)}, "spacing"),
    (GOOD, {"spacing": (1.0, float("inf"), 1.0)}, "spacing"),
    (GOOD, {"spacing": (1.0, 1.0)}, "spacing"),
    (GOOD, {"origin": (0.0, float("nan"), 0.0)}, "origin"),
    (GOOD, {}, "HIP device"),                          # a host tensor: refused last, there is no CPU path
])
def test_marching_tetrahedra_value_errors(field, kw, what):
    kw = dict(kw)
    iso = kw.pop("iso", 0.0)
    with pytest.raises(ValueError, match=what.replace("(", r"\(").replace(")", r"\)")):
        mesh.marching_tetrahedra(field, iso, **kw)


def _cpu_nets():
    from nerf_amd.addtional import ProposalNetwork
    from nerf_amd.mip_model import MipNeRF
    return ProposalNetwork(10, 256), MipNeRF(10, 4, 256)


BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


@pytest.mark.parametrize("kw,what", [
    (dict(network=torch.nn.Linear(3, 1)), "MipNeRF, a ProposalNetwork or a RefNeRF"),
    (dict(resolution=1), "resolution"),
    (dict(resolution=(4, 4)), "resolution"),
    (dict(resolution=(4, 1, 4)), "resolution"),
    (dict(aabb=((0, 0, 0), (1, 1, 0))), "aabb"),
    (dict(aabb=((0, 0, 0), (1, 1))), "aabb"),
    (dict(aabb=((0, 0, 0), (1, float("nan"), 1))), "aabb"),
    (dict(activation="relu"), "activation"),
    (dict(chunk_points=0), "chunk_points"),
    (dict(resolution=(2048, 2048, 512)), "2\\^31"),
])
def test_density_grid_value_errors(kw, what):
    prop, _ = _cpu_nets()
    args = dict(network=prop, aabb=BOX, resolution=4)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        mesh.density_grid(args.pop("network"), args.pop("aabb"), args.pop("resolution"), **args)


def test_extract_mesh_refuses_colours_of_a_proposal_network():
    prop, _ = _cpu_nets()
    with pytest.raises(ValueError, match="colour"):
        mesh.extract_mesh(prop, BOX, 4, 0.0, colors=True)


def test_scan_step_constant_mirrors_the_header():
    import os
    import re
    from nerf_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_amd.h")).read()
    assert int(re.search(r"#define NERF_AMD_MESH_SCAN_STEP_TILES (\d+)", header).group(1)) == _lib.MESH_SCAN_STEP_TILES
    tiles = (R.gyroid_field().size + 255) // 256                      # the lattice of the GPU test that takes the scan through two steps
    assert _lib.MESH_SCAN_STEP_TILES < tiles < 2 * _lib.MESH_SCAN_STEP_TILES and tiles % 1024 not in (0, 1023)


def test_render_only_parser_has_the_mesh_flags_off_by_default():
    from nerf_amd import procedures
    a = procedures.get_parser().parse_args([])
    assert a.mesh is None and a.mesh_res == 256 and a.mesh_iso == 10.0 and a.mesh_aabb == [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    a = procedures.get_parser().parse_args(["--mesh", "out.ply", "--mesh_res", "64", "--mesh_iso", "2.5", "--mesh_aabb", "-1", "-2", "-3", "1", "2", "3"])
    assert (a.mesh, a.mesh_res, a.mesh_iso, a.mesh_aabb) == ("out.ply", 64, 2.5, [-1.0, -2.0, -3.0, 1.0, 2.0, 3.0])
