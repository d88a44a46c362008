"""Triangle meshes from the density field, on the device: marching tetrahedra (nerf_amd_mesh_count / nerf_amd_mesh_emit; the definition is
in include/nerf_amd.h and, in fp64, in tests/mesh_ref.py) on a lattice of densities that the networks' own forwards fill in.

    field, origin, spacing = density_grid(mip_net, ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)), 256)
    mesh = marching_tetrahedra(field, 10.0, origin=origin, spacing=spacing)
    write_ply("lego.ply", mesh["vertices"], mesh["faces"], mesh["normals"])

or extract_mesh(...) for the two in one call, with per-vertex colours from one more forward."""
import numpy as np
import torch

from . import ops

_VIEW_DIR = (0.0, 0.0, -1.0)           # the constant view direction of the density pass (density does not depend on it)


def marching_tetrahedra(field: torch.Tensor, iso: float, *, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals: bool = True):
    """The iso-surface { field = iso } of an fp32 device lattice (nz, ny, nx), x fastest; lattice point (i, j, k) sits at
    origin + spacing * (i, j, k).  -> {"vertices" (V,3) fp32, "faces" (F,3) int32[, "normals" (V,3) fp32]}, device tensors: vertices in
    ascending (point, edge slot) order, faces in (cell, tetrahedron, triangle) order, wound so that the normal points from high values
    to low.  One host read (the two counts) between the counting and the emitting launches; an empty surface launches no emit pass.
    ValueError, before anything is launched, for a field that is not a contiguous fp32 device tensor of rank 3."""
    ops._mesh_args(field, iso, origin, spacing, "nerf_amd.marching_tetrahedra")
    counts, ws = ops.mesh_count(field, iso)
    n_vertices, n_faces = (int(v) for v in counts.tolist())
    vertices, faces, nrm = ops.mesh_emit(field, iso, ws, n_vertices, n_faces, origin=origin, spacing=spacing, normals=normals)
    out = {"vertices": vertices, "faces": faces}
    if normals:
        out["normals"] = nrm
    return out


def _network_kind(network):
    from .addtional import ProposalNetwork
    from .mip_model import MipNeRF
    from .ref_model import RefNeRF
    for kind, cls in (("ref", RefNeRF), ("mip", MipNeRF), ("proposal", ProposalNetwork)):
        if isinstance(network, cls):
            return kind
    raise ValueError("nerf_amd.mesh: the network must be a MipNeRF, a ProposalNetwork or a RefNeRF (got %s)" % type(network).__name__)


def _resolution(resolution):
    res = (int(resolution),) * 3 if isinstance(resolution, (int, np.integer)) else tuple(int(v) for v in resolution)
    if len(res) != 3 or min(res) < 2:
        raise ValueError("nerf_amd.mesh: resolution is an int or (nx, ny, nz), every entry at least 2 (got %r)" % (resolution,))
    return res


def _aabb(aabb):
    try:
        box = np.asarray(aabb, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        box = np.zeros(0)
    if box.size != 6 or not np.isfinite(box).all() or not (box[3:] > box[:3]).all():
        raise ValueError("nerf_amd.mesh: aabb is (min xyz, max xyz) with min < max (got %r)" % (aabb,))
    return box[:3], box[3:]


def _forward(network, kind, pos, dirs, contract):
    """the network's own forward on (n, 3) positions [and directions] -> ((n,) raw sigma, (n, 3) rgb or None)"""
    if kind == "proposal":
        return network(pos.view(-1, 1, 3), contract=contract).reshape(-1), None
    pts = torch.cat((pos, dirs), dim=-1).view(-1, 1, 6)
    out = network(pts, contract=contract)
    rgbo = (out[0] if kind == "ref" else out).reshape(-1, 4)
    return rgbo[:, 3], rgbo[:, :3]


def _activate(sigma, kind, activation):
    if activation == "raw":
        return sigma
    return torch.nn.functional.softplus(sigma + 0.5) if kind == "ref" else torch.relu(sigma)      # what compositing applies


def density_grid(network, aabb, resolution, *, contract: bool = False, activation: str = "render", chunk_points: int = 1 << 22):
    """The network's density on the lattice of `resolution` = n or (nx, ny, nz) points per axis that spans `aabb` = (min xyz, max xyz):
    point i of an axis sits at min + (max - min) i / (n - 1) (evaluated in fp64, rounded to fp32).  -> (field (nz, ny, nx) fp32 on the
    network's device, origin (3 floats), spacing (3 floats)).  sigma comes from the network's existing forward, `chunk_points` points at
    a time, under no_grad: column 3 of MipNeRF / RefNeRF's forward with the constant view direction (0, 0, -1), ProposalNetwork's forward.
    activation "render": what compositing applies (ReLU; softplus(sigma + 0.5) for Ref-NeRF); "raw": nothing."""
    kind = _network_kind(network)
    nx, ny, nz = _resolution(resolution)
    lo, hi = _aabb(aabb)
    if activation not in ("render", "raw"):
        raise ValueError("nerf_amd.mesh: activation is 'render' or 'raw' (got %r)" % (activation,))
    chunk_points = int(chunk_points)
    if chunk_points < 1:
        raise ValueError("nerf_amd.mesh: chunk_points must be positive (got %d)" % chunk_points)
    n = nx * ny * nz
    if n >= 2 ** 31:
        raise ValueError("nerf_amd.mesh: nx * ny * nz must stay below 2^31 (got %r)" % ((nx, ny, nz),))
    dev = next(network.parameters()).device
    axes = [torch.from_numpy((lo[a] + (hi[a] - lo[a]) * np.arange(m, dtype=np.float64) / (m - 1)).astype(np.float32)).to(dev) for a, m in enumerate((nx, ny, nz))]
    field = torch.empty((n,), dtype=torch.float32, device=dev)
    view = torch.tensor(_VIEW_DIR, dtype=torch.float32, device=dev)
    with torch.no_grad():
        for first in range(0, n, chunk_points):
            p = torch.arange(first, min(first + chunk_points, n), dtype=torch.int64, device=dev)
            row = torch.div(p, nx, rounding_mode="floor")
            pos = torch.stack((axes[0][p - row * nx], axes[1][row % ny], axes[2][torch.div(row, ny, rounding_mode="floor")]), dim=-1)
            sigma, _ = _forward(network, kind, pos, view.expand(pos.shape[0], 3), contract)
            field[first:first + pos.shape[0]] = _activate(sigma.float(), kind, activation)
    origin = tuple(float(np.float32(v)) for v in lo)
    spacing = tuple(float(np.float32((hi[a] - lo[a]) / (m - 1))) for a, m in enumerate((nx, ny, nz)))
    return field.view(nz, ny, nx), origin, spacing


def extract_mesh(network, aabb, resolution, iso: float, *, contract: bool = False, colors: bool = False, activation: str = "render",
                 chunk_points: int = 1 << 22):
    """density_grid followed by marching_tetrahedra -> {"vertices", "faces", "normals"[, "colors"]}.  colors=True (MipNeRF, RefNeRF): one
    more forward at the vertex positions, looking at the surface head-on (view direction -n; (0, 0, -1) where n is zero) -> "colors"
    (V, 3) fp32.  A ProposalNetwork has no colour: ValueError."""
    kind = _network_kind(network)
    if colors and kind == "proposal":
        raise ValueError("nerf_amd.extract_mesh: colors=True needs a MipNeRF or a RefNeRF (a ProposalNetwork has no colour output)")
    field, origin, spacing = density_grid(network, aabb, resolution, contract=contract, activation=activation, chunk_points=chunk_points)
    mesh = marching_tetrahedra(field, iso, origin=origin, spacing=spacing, normals=True)
    if colors:
        mesh["colors"] = _vertex_colors(network, kind, mesh["vertices"], mesh["normals"], contract, chunk_points)
    return mesh


def _vertex_colors(network, kind, vertices: torch.Tensor, normals: torch.Tensor, contract: bool, chunk_points: int):
    """(V, 3) fp32: the rgb of the network's forward at the vertices with view direction -normal ((0, 0, -1) where the normal is zero)"""
    view = torch.tensor(_VIEW_DIR, dtype=torch.float32, device=vertices.device)
    dirs = torch.where((normals == 0).all(dim=-1, keepdim=True), view, -normals)
    out = torch.empty((vertices.shape[0], 3), dtype=torch.float32, device=vertices.device)
    with torch.no_grad():
        for first in range(0, vertices.shape[0], int(chunk_points)):
            last = min(first + int(chunk_points), vertices.shape[0])
            out[first:last] = _forward(network, kind, vertices[first:last], dirs[first:last], contract)[1].float()
    return out


def write_ply(path, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY: per vertex float x y z [nx ny nz] [uchar red green blue, from `colors` clipped to [0, 1]]; per face
    uchar 3 + three int32.  Tensors (any device) or arrays."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v = np.ascontiguousarray(to_np(vertices), dtype="<f4")
    f = np.ascontiguousarray(to_np(faces), dtype="<i4")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError("nerf_amd.write_ply: vertices are (V, 3) and faces (F, 3) (got %s and %s)" % (v.shape, f.shape))
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    cols = [v]
    if normals is not None:
        nrm = np.ascontiguousarray(to_np(normals), dtype="<f4")
        if nrm.shape != v.shape:
            raise ValueError("nerf_amd.write_ply: normals must be (V, 3) like the vertices (got %s)" % (nrm.shape,))
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        cols.append(nrm)
    rgb = None
    if colors is not None:
        c = to_np(colors).astype(np.float64)
        if c.shape != v.shape:
            raise ValueError("nerf_amd.write_ply: colors must be (V, 3) like the vertices (got %s)" % (c.shape,))
        rgb = np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vrec = np.empty(v.shape[0], dtype=fields)
    for block, names in zip(cols, (("x", "y", "z"), ("nx", "ny", "nz"))):
        for q, name in enumerate(names):
            vrec[name] = block[:, q]
    if rgb is not None:
        for q, name in enumerate(("red", "green", "blue")):
            vrec[name] = rgb[:, q]
    frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"] = 3
    frec["v"] = f
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]]
    header += ["property %s %s" % ("uchar" if t == "u1" else "float", name) for name, t in fields]
    header += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(vrec.tobytes())
        out.write(frec.tobytes())
