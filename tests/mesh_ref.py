"""fp64 specification of the iso-surface extraction (nerf_amd_mesh_count / nerf_amd_mesh_emit, include/nerf_amd.h), its comparator, the
bounds on what the fp32 kernel may differ by, and the test fields.

The specification is written WITHOUT a case table: every tetrahedron goes through the one generic rule of the header -- sort its corners
into inside (ascending) and outside (ascending), emit by |I|, orient by the integer midpoint test -- vectorised over all cells of one Kuhn
tetrahedron at a time.  The kernel's 6 x 16 table is derived in C++ at compile time; the two share no code and no typed-in entry.

Topology is decided on the fp32 values (f >= iso), so spec and kernel must agree on counts and faces EXACTLY; positions and normals are
evaluated here in fp64 and compared within the bounds derived below from the arithmetic that mesh_kernels.hip ships (u = 2^-24):

  position, per axis with direction bit d, lattice index a, spacing h, origin o (all exact fp32 inputs):
      t = fl(fl(iso - f_a) / fl(f_b - f_a))   three roundings of exact inputs, each relative      |dt| <= 3.01 u t   (t <= 1; the clamp adds none)
                                              (a subnormal difference is exact; a subnormal quotient adds 2^-149, the TINY term)
      c = fl(a + t)   (only where d = 1)                                                          u (a + t)
      fl(h c)                                                                                     u h c
      fl(o + .)                                                                                   u |position|
      bound = h d (3.01 u t + u (a + t) + TINY) + u h c + u |position|, times 1.001 for the second-order terms.
  normal: g = fl(fl(f_hi - f_lo) / (h (hi - lo)))  relative 2 u  (h (hi - lo) is exact);  w0 = fl(1 - t): |dw0| <= u + 3.01 u
      v = fl(fl(w0 g_a) + fl(t g_b)) per axis:  |dv| <= |g_a| (4.01 u + 3 u) + |g_b| (3.01 u + 3 u) + u (|g_a| + |g_b|) <= 8.01 u (|g_a| + |g_b|)
      E = the 2-norm of that over the axes.  |normalize(v + e) - normalize(v)| <= 2 |e| / |v|; the normalisation itself (three squares,
      two sums, a root, a division) moves a unit vector by less than 8 u.
      bound = 2 E / |v| + 8 u;  infinite (the check is vacuous, and the comparator only asks for a finite vector of length <= 1) where
      |v| is 0, not finite, or outside [1e-15, 1e15] (the fp32 squares may leave the normal range there).
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
VACUOUS = 0.1                      # a normal bound at or above this checks nothing worth the name

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))        # axis 0 = x; lexicographic: xyz xzy yxz yzx zxy zyx
FAULTS = ("quad_diagonal", "tet_order", "t_from_b", "no_flip", "slot_off_by_one", "no_clamp", "spacing_axis")


def slot_direction(s, fault=None):
    c = s + 1
    if fault == "slot_off_by_one":
        c = (s + 1) % 7 + 1
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def tet_corners(perm):
    """(4, 3) integer offsets (dx, dy, dz) of v0..v3"""
    c = [np.zeros(3, dtype=np.int64)]
    for ax in perm:
        nxt = c[-1].copy()
        nxt[ax] += 1
        c.append(nxt)
    return np.stack(c)


def gradient(f, spacing):
    """(nz, ny, nx, 3): central differences inside, one-sided on the faces, each axis divided by its spacing (component 0 = x)"""
    g = np.zeros(f.shape + (3,))
    with np.errstate(all="ignore"):
        for comp, axis in ((0, 2), (1, 1), (2, 0)):
            n = f.shape[axis]
            idx = np.arange(n)
            lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
            diff = np.take(f, hi, axis=axis) - np.take(f, lo, axis=axis)
            shape = [1, 1, 1]
            shape[axis] = n
            g[..., comp] = diff / (spacing[comp] * (hi - lo).reshape(shape))
    return g


def spec(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), fault=None):
    """-> dict: vertices (V,3) f64, normals (V,3) f64, faces (F,3) int32, pos_bound (V,3), normal_bound (V,)"""
    assert fault is None or fault in FAULTS
    f32 = np.ascontiguousarray(field, dtype=np.float32)
    nz, ny, nx = f32.shape
    iso32 = np.float32(iso)
    inside = f32 >= iso32                                             # NaN: False
    f = f32.astype(np.float64)
    iso = float(iso32)
    origin = np.asarray([float(np.float32(v)) for v in origin])
    spacing = np.asarray([float(np.float32(v)) for v in spacing])

    # ---- vertices: ascending (p, s)
    cross = np.zeros((nz, ny, nx, 7), dtype=bool)
    dirs = [slot_direction(s, fault) for s in range(7)]
    for s, (dx, dy, dz) in enumerate(dirs):
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        cross[:nz - dz, :ny - dy, :nx - dx, s] = a != b
    flat = cross.reshape(-1, 7)
    edge_id = np.where(flat, np.cumsum(flat.reshape(-1)).reshape(-1, 7) - 1, -1)
    slot_of_code = np.full(8, -1, dtype=np.int64)
    for s, (dx, dy, dz) in enumerate(dirs):
        slot_of_code[dx + 2 * dy + 4 * dz] = s
    p_idx, s_idx = np.nonzero(flat)
    ai = np.stack((p_idx % nx, (p_idx // nx) % ny, p_idx // (nx * ny)), axis=1)          # (V, 3): i, j, k
    d = np.asarray(dirs, dtype=np.int64)[s_idx]
    bi = ai + d
    fa = f[ai[:, 2], ai[:, 1], ai[:, 0]]
    fb = f[bi[:, 2], bi[:, 1], bi[:, 0]]
    with np.errstate(all="ignore"):
        t = (iso - fb) / (fa - fb) if fault == "t_from_b" else (iso - fa) / (fb - fa)
        if fault != "no_clamp":                 # the clamp and the non-finite rule are one step; see test_mesh_host for what this fault can show
            t = np.where(np.isfinite(t), np.clip(t, 0.0, 1.0), 0.5)
    use_spacing = spacing.copy()
    if fault == "spacing_axis":
        use_spacing[1] = 1.0
    with np.errstate(all="ignore"):
        c = ai + t[:, None] * d
        vertices = origin + use_spacing * c
        pos_bound = 1.001 * (spacing * d * (3.01 * U * t[:, None] + U * (ai + t[:, None]) + TINY) + U * spacing * c + U * np.abs(vertices))

        # ---- normals
        g = gradient(f, spacing)
        ga, gb = g[ai[:, 2], ai[:, 1], ai[:, 0]], g[bi[:, 2], bi[:, 1], bi[:, 0]]
        v = (1.0 - t)[:, None] * ga + t[:, None] * gb
        length = np.sqrt((v * v).sum(1))
        good = np.isfinite(length) & (length > 0.0)
        normals = np.where(good[:, None], -v / np.where(good, length, 1.0)[:, None], 0.0)
        E = 8.01 * U * np.sqrt(((np.abs(ga) + np.abs(gb)) ** 2).sum(1))
        measurable = good & (length >= 1e-15) & (length <= 1e15) & np.isfinite(E)
        normal_bound = np.where(measurable, 2.0 * E / np.where(measurable, length, 1.0) + 8.0 * U, np.inf)

    # ---- faces: one generic rule per tetrahedron
    # (only cells whose eight corners are not all on one side can hold a triangle; they are visited in ascending p)
    n_in = sum(inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int8) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1))
    ck, cj, ci = np.nonzero((n_in > 0) & (n_in < 8))
    cell_p = (ck * ny + cj) * nx + ci
    perms = list(PERMS)
    if fault == "tet_order":
        perms[0], perms[1] = perms[1], perms[0]
    keys, tris = [], []
    for t_no, perm in enumerate(perms):
        cp = tet_corners(perm)                                                   # (4, 3)
        ins = np.stack([inside[ck + cp[l, 2], cj + cp[l, 1], ci + cp[l, 0]] for l in range(4)], axis=1)
        order = np.argsort(~ins, axis=1, kind="stable")                        # the inside corners ascending, then the outside ones ascending
        ni = ins.sum(1)
        batches = []
        for count, a_col, rest in ((1, 0, (1, 2, 3)), (3, 3, (0, 1, 2))):
            sel = np.nonzero(ni == count)[0]
            a = order[sel, a_col]
            batches.append((sel, 0, np.stack((a, a, a), 1), order[sel][:, list(rest)]))
        sel = np.nonzero(ni == 2)[0]
        a, b, c_, d_ = (order[sel, q] for q in range(4))
        if fault == "quad_diagonal":
            batches.append((sel, 0, np.stack((a, a, b), 1), np.stack((c_, d_, c_), 1)))
            batches.append((sel, 1, np.stack((a, b, b), 1), np.stack((d_, d_, c_), 1)))
        else:
            batches.append((sel, 0, np.stack((a, a, b), 1), np.stack((c_, d_, d_), 1)))
            batches.append((sel, 1, np.stack((a, b, b), 1), np.stack((c_, d_, c_), 1)))
        for sel, k_no, Uc, Wc in batches:
            if sel.size == 0:
                continue
            mid2 = cp[Uc] + cp[Wc]                                              # (m, 3, 3): twice the edge midpoints
            insb = ins[sel].astype(np.int64)
            n_in = insb.sum(1, keepdims=True)
            towards_out = n_in * ((1 - insb) @ cp) - (4 - n_in) * (insb @ cp)   # (mean outside - mean inside) * |I| * |O|
            s = (np.cross(mid2[:, 1] - mid2[:, 0], mid2[:, 2] - mid2[:, 0]) * towards_out).sum(1)
            assert (s != 0).all(), "the orientation test is never degenerate"
            if fault != "no_flip":
                flip = s < 0
                Uc, Wc = Uc.copy(), Wc.copy()
                Uc[flip, 1], Uc[flip, 2] = Uc[flip, 2], Uc[flip, 1].copy()
                Wc[flip, 1], Wc[flip, 2] = Wc[flip, 2], Wc[flip, 1].copy()
            lo, hi = np.minimum(Uc, Wc), np.maximum(Uc, Wc)
            own = cp[lo]                                                        # (m, 3, 3)
            dd = cp[hi] - own
            slot = slot_of_code[dd[..., 0] + 2 * dd[..., 1] + 4 * dd[..., 2]]
            p_own = ((ck[sel, None] + own[..., 2]) * ny + (cj[sel, None] + own[..., 1])) * nx + (ci[sel, None] + own[..., 0])
            vid = edge_id[p_own, slot]
            assert (vid >= 0).all()
            tris.append(vid)
            keys.append((cell_p[sel] * 6 + t_no) * 2 + k_no)
    if tris:
        key = np.concatenate(keys)
        faces = np.concatenate(tris)[np.argsort(key, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    return {"vertices": vertices, "normals": normals, "faces": faces.reshape(-1, 3), "pos_bound": pos_bound, "normal_bound": normal_bound, "t": t,
            "owner": ai, "direction": d}


def shipped_arithmetic(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """The vertex and normal arithmetic of mesh_kernels.hip restated operation by operation in numpy float32 (IEEE, no contraction), on the
    spec's own vertex list: what the bounds above have to cover, checked on the host before any device is involved."""
    sp = spec(field, iso, origin, spacing)
    f = np.ascontiguousarray(field, dtype=np.float32)
    a, d = sp["owner"], sp["direction"]
    b = a + d
    one, zero, half = np.float32(1.0), np.float32(0.0), np.float32(0.5)
    o32, s32 = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
    fa, fb = f[a[:, 2], a[:, 1], a[:, 0]], f[b[:, 2], b[:, 1], b[:, 0]]
    with np.errstate(all="ignore"):
        t = (np.float32(iso) - fa) / (fb - fa)
        t = np.where(np.isfinite(t), np.minimum(np.maximum(t, zero), one), half).astype(np.float32)
        af = a.astype(np.float32)
        c = np.where(d == 1, af + t[:, None], af).astype(np.float32)
        vertices = o32 + s32 * c
        g = np.zeros(f.shape + (3,), dtype=np.float32)
        for comp, axis in ((0, 2), (1, 1), (2, 0)):
            n = f.shape[axis]
            idx = np.arange(n)
            lo, hi = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
            shape = [1, 1, 1]
            shape[axis] = n
            g[..., comp] = (np.take(f, hi, axis=axis) - np.take(f, lo, axis=axis)) / (s32[comp] * (hi - lo).astype(np.float32).reshape(shape))
        ga, gb = g[a[:, 2], a[:, 1], a[:, 0]], g[b[:, 2], b[:, 1], b[:, 0]]
        w0 = one - t
        v = w0[:, None] * ga + t[:, None] * gb
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        good = (length > zero) & np.isfinite(length)
        normals = np.where(good[:, None], -(v / np.where(good, length, one)[:, None]), zero).astype(np.float32)
    assert vertices.dtype == np.float32 and v.dtype == np.float32
    return {"vertices": vertices, "normals": normals, "faces": sp["faces"].copy()}


def read_ply(path):
    """a reader for what nerf_amd.mesh.write_ply writes (binary little-endian; float / uchar vertex properties, uchar-counted int faces)
    -> (dict of vertex property arrays, faces (F, 3) int32)"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    counts, props, element = {}, [], None
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            element = w[1]
            counts[element] = int(w[2])
        elif w[0] == "property" and element == "vertex":
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
        elif w[0] == "property":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"], line
    vdt = np.dtype(props)
    vrec = np.frombuffer(data, dtype=vdt, count=counts["vertex"], offset=end)
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    frec = np.frombuffer(data, dtype=fdt, count=counts["face"], offset=end + vdt.itemsize * counts["vertex"])
    assert end + vdt.itemsize * counts["vertex"] + fdt.itemsize * counts["face"] == len(data), "trailing or missing bytes"
    assert (frec["n"] == 3).all()
    return {name: vrec[name].copy() for name, _ in props}, frec["v"].astype(np.int32)


def compare(got, want, normals=True):
    """`got` (vertices, faces[, normals]: arrays) against spec()'s `want` -> (list of complaints, worst position error / bound, worst
    normal error / bound over the vertices with a finite bound).  An empty list is a pass."""
    bad = []
    gv, gf = np.asarray(got["vertices"], dtype=np.float64), np.asarray(got["faces"])
    if gv.shape != want["vertices"].shape:
        return ["vertex count %s, want %s" % (gv.shape, want["vertices"].shape)], np.inf, np.inf
    if gf.shape != want["faces"].shape:
        return ["face count %s, want %s" % (gf.shape, want["faces"].shape)], np.inf, np.inf
    if gf.dtype != np.int32:
        bad.append("faces are %s, want int32" % gf.dtype)
    if not np.array_equal(gf, want["faces"]):
        first = int(np.nonzero((gf != want["faces"]).any(1))[0][0])
        bad.append("faces differ, first at %d: %s, want %s" % (first, gf[first], want["faces"][first]))
    pos_ratio = nrm_ratio = 0.0
    if gv.size:
        if not np.isfinite(gv).all():
            bad.append("a vertex position is not finite")
        else:
            err = np.abs(gv - want["vertices"])                 # (a coordinate that is exactly 0 has the bound 0: it must be reproduced exactly)
            ratio = np.divide(err, want["pos_bound"], out=np.where(err > 0.0, np.inf, 0.0), where=want["pos_bound"] > 0.0)
            pos_ratio = float(ratio.max())
            if pos_ratio > 1.0:
                at = np.unravel_index(int(ratio.argmax()), ratio.shape)
                bad.append("vertex %d axis %d: %r, want %r (error / bound %.3g)" % (at[0], at[1], gv[at], want["vertices"][at], pos_ratio))
    if normals and gv.size:
        gn = np.asarray(got["normals"], dtype=np.float64)
        if gn.shape != want["normals"].shape:
            bad.append("normals are %s, want %s" % (gn.shape, want["normals"].shape))
        elif not np.isfinite(gn).all() or (np.sqrt((gn * gn).sum(1)) > 1.0 + 1e-5).any():
            bad.append("a normal is not finite or longer than 1")
        else:
            err = np.sqrt(((gn - want["normals"]) ** 2).sum(1))
            fin = np.isfinite(want["normal_bound"])
            if fin.any():
                ratio = err[fin] / want["normal_bound"][fin]
                nrm_ratio = float(ratio.max())
                if nrm_ratio > 1.0:
                    at = int(np.nonzero(fin)[0][int(ratio.argmax())])
                    bad.append("normal %d: %s, want %s (error / bound %.3g)" % (at, gn[at], want["normals"][at], nrm_ratio))
    return bad, pos_ratio, nrm_ratio


# ---------------------------------------------------------------------------------------------------------------- mesh properties
def edge_census(faces):
    """directed edges of the faces -> (every undirected edge is in exactly two faces, once in each direction; V used, E, F)"""
    faces = np.asarray(faces, dtype=np.int64)
    e = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    n = int(faces.max()) + 1 if faces.size else 0
    directed = e[:, 0] * n + e[:, 1]
    und = np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1])
    _, d_counts = np.unique(directed, return_counts=True)
    _, u_counts = np.unique(und, return_counts=True)
    closed = bool((d_counts == 1).all() and (u_counts == 2).all())
    return closed, len(np.unique(faces)), len(u_counts), len(faces)


def euler_characteristic(faces):
    _, v, e, f = edge_census(faces)
    return v - e + f


def boundary_edges(faces):
    """(m, 2) vertex ids of the undirected edges that only one face uses"""
    faces = np.asarray(faces, dtype=np.int64)
    e = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    e = np.sort(e, axis=1)
    uniq, counts = np.unique(e, axis=0, return_counts=True)
    return uniq[counts == 1]


def signed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    p0, p1, p2 = (v[np.asarray(faces)[:, q]] for q in range(3))
    return float((p0 * np.cross(p1, p2)).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------------------- fields
def _grid(shape):
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return x, y, z


def sphere_field(shape=(13, 12, 11)):
    x, y, z = _grid(shape)
    return (3.3 ** 2 - ((x - 5.1) ** 2 + (y - 5.4) ** 2 + (z - 6.2) ** 2)).astype(np.float32)


def torus_field(shape=(9, 15, 16)):
    x, y, z = _grid(shape)
    return (1.6 ** 2 - ((np.sqrt((x - 7.6) ** 2 + (y - 7.2) ** 2) - 4.3) ** 2 + (z - 4.1) ** 2)).astype(np.float32)


def two_spheres_field(shape=(9, 9, 17)):
    x, y, z = _grid(shape)
    a = 2.2 ** 2 - ((x - 4.2) ** 2 + (y - 4.1) ** 2 + (z - 4.3) ** 2)
    b = 2.1 ** 2 - ((x - 12.4) ** 2 + (y - 4.3) ** 2 + (z - 4.2) ** 2)
    return np.maximum(a, b).astype(np.float32)


def noise_field(shape, seed=7):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def gyroid_field(shape=(97, 105, 112), periods=(23.0, 19.0, 29.0)):
    """a gyroid: surface in every part of the lattice, so every scan tile carries counts.  The default has 1 140 720 points = 4 456
    tiles of 256: two steps of the tile scan (4 096 tiles each), all four groups and all four waves of the first one."""
    x, y, z = _grid(shape)
    a, b, c = (2.0 * np.pi / p for p in periods)
    return (np.sin(a * x) * np.cos(b * y) + np.sin(b * y) * np.cos(c * z) + np.sin(c * z) * np.cos(a * x)).astype(np.float32)


def integer_ball_field(shape=(11, 11, 13)):
    """a ball rounded to integers (many f == iso at iso 0) inside a shell of outside values"""
    x, y, z = _grid(shape)
    nz, ny, nx = shape
    f = np.rint(3.0 ** 2 - ((x - (nx - 1) / 2.0) ** 2 + (y - (ny - 1) / 2.0) ** 2 + (z - (nz - 1) / 2.0) ** 2))
    return f.astype(np.float32)


def specials_field(shape=(6, 7, 8), seed=11):
    f = noise_field(shape, seed)
    f[2, 3, 4] = np.nan
    f[3, 2, 5] = np.inf
    f[1, 4, 2] = -np.inf
    return f


CLOSED = {"sphere": (sphere_field, 2), "torus": (torus_field, 0), "two_spheres": (two_spheres_field, 4)}
