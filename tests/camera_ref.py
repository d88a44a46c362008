"""The camera model of include/nerf_amd.h in fp64 -- pixel -> (xd, yd), the forward (OpenCV / COLMAP) model, the fixed-step Newton inverse,
the ray -- an operation-by-operation fp32 restatement of the kernels' arithmetic for planting faults on the host, and the two bounds the
GPU tests hold the kernels to.  Nothing here is fitted to what the kernels return.

THE BOUNDS.  The build contracts nothing (-ffp-contract=off) and its fp32 divisions are correctly rounded, so every kernel operation
is one IEEE rounding: |fl(v) - v| <= h(v) := half an ulp of the binade of v (<= 2^-24 |v|, up to 2 x sharper).  `_Run` carries a value
together with a bound on the error of its fp32 evaluation: for z = a op b, err(z) = propagated input errors + h(|z| + err).

(1) Backward error, reference-free.  Let x' be the iterate before the LAST Newton step, rh the kernel's computed residual there (against
its own fp32 pixel point xdh), dh its computed correction, and x_N = fl(x' - dh) the point it returns.  In exact arithmetic
    F(x_N) - xd = (F(x') - xdh - rh)        (a) the fp32 rounding of ONE residual evaluation: `_Run` through the kernel's expression,
                + (rh - J dh)               (b) the rounding of the 2x2 solve, proportional to |dh|,
                - J eta                     (c) eta = the rounding of the final subtraction, |eta| <= h(x_N) per component,
                + R2                        (d) Taylor remainder, |R2| <= M |dh|^2 (M bounds the forward model's second derivatives),
                + (xdh - xd)                (e) the pixel map: COMPUTED, not bounded -- the header fixes its grouping, so xdh is specified.
(b) and (d) need the last correction to be small: |dh| <= DELTA_LAST = 2^-16.  That is a condition on the CAMERA (Newton has
converged to the fp32 floor one step before the end), checked for every test camera by tests/test_camera_host.py on the fp32 restatement
below.  Under it (b) <= 64 * 2^-24 * DELTA_LAST (each component of dh carries < 8 roundings, amplified by cond(J) <= 8 where det J > 0.3
and |J_ij| <= 1.5) and (d) <= M DELTA_LAST^2 with M = 4 (6 |k1| R + 20 |k2| R^3 + 42 |k3| R^5 + 6 (|p1| + |p2|)), R the largest |x|, |y|
(the second partials of x rad(r2) are 6 x rad' + 4 x^3 rad'' and smaller mixed ones; four of them meet in a component of the form) --
together below 1e-9, three hundred times under (a).  (a) is evaluated at x_N instead of x' (they differ by <= DELTA_LAST; the bound is
Lipschitz): inflated by 1 + 2^-8.
(2) Direction.  With x* the fp64 root, x_N - x* = J^-1 (F(x_N) - xd) to first order: |x_N - x*| <= |J^-1| B (1 + 2^-8) elementwise, B the
bound (1); pushed through d_i = fl(fl(fl(x R_i0) + fl(-y R_i1)) + (-R_i2)) with `_Run` (the product by -1 is exact)."""
import numpy as np

NEWTON_STEPS = 3              # NERF_AMD_CAMERA_NEWTON_STEPS
DET_EPS = 1e-6                # NERF_AMD_CAMERA_DET_EPS
DELTA_LAST = 2.0 ** -16
U = 2.0 ** -24


def h(v):
    """half an ulp (fp32) of the binade of |v|, v fp64: the largest rounding error of an fp32 result of that size (normal range)"""
    v = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 24.0)


class _Run:
    """value (fp64) + a bound on the error of its fp32 evaluation"""

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, dtype=np.float64), np.asarray(e, dtype=np.float64)

    @staticmethod
    def _of(x):
        return x if isinstance(x, _Run) else _Run(x)

    def _rounded(self, v, e):
        return _Run(v, e + h(np.abs(v) + e))

    def __mul__(self, o):
        o = _Run._of(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __add__(self, o):
        o = _Run._of(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = _Run._of(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def twice(self):
        return _Run(2.0 * self.v, 2.0 * self.e)        # exact in binary


def row32(cam):
    """the camera row as the kernel sees it: fp32 values, in fp64"""
    r = np.asarray(cam.row() if hasattr(cam, "row") else cam, dtype=np.float32).astype(np.float64)
    assert r.shape == (12,)
    return r


def pixel_plane(row, cols, rows):
    """(xd, yd) of the pixel centres in fp64 (the real-number value of the header's expression on the fp32 row)"""
    return (np.asarray(cols, np.float64) + 0.5 - row[2]) / row[0], (np.asarray(rows, np.float64) + 0.5 - row[3]) / row[1]


def pixel_plane32(row, cols, rows):
    """the same in the header's fp32 grouping, every operation rounded: what the kernel is SPECIFIED to compute (returned in fp64)"""
    r = row.astype(np.float32)
    xd = ((np.asarray(cols).astype(np.float32) + np.float32(0.5)) - r[2]) / r[0]
    yd = ((np.asarray(rows).astype(np.float32) + np.float32(0.5)) - r[3]) / r[1]
    return xd.astype(np.float64), yd.astype(np.float64)


def distort(row, x, y):
    k1, k2, k3, p1, p2 = row[4:9]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * rad + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)


def jacobian(row, x, y):
    """(jxx, jxy, jyy) of the forward model; jyx = jxy"""
    k1, k2, k3, p1, p2 = row[4:9]
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (2.0 * k2 + r2 * 3.0 * k3)
    return (rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x, 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y,
            rad + 2.0 * y * y * drad + 2.0 * p2 * x + 6.0 * p1 * y)


def undistort(row, xd, yd, steps=NEWTON_STEPS, dtype=np.float64, drop_k3=False, swap_p=False, last=None):
    """`steps` Newton steps from (xd, yd), every one taken unless |det| < DET_EPS; none when the five coefficients are zero.  dtype
    float64: the specification.  dtype float32: the kernels' arithmetic operation by operation in their grouping (`drop_k3`, `swap_p`:
    planted faults).  `last`: a list that receives the largest |correction| of the last step."""
    t = dtype
    k1, k2, k3, p1, p2 = (t(v) for v in row[4:9])
    if drop_k3:
        k3 = t(0)
    if swap_p:
        p1, p2 = p2, p1
    xd, yd = np.asarray(xd).astype(t), np.asarray(yd).astype(t)
    x, y = xd.copy(), yd.copy()
    if not any(float(v) != 0.0 for v in (k1, k2, k3, p1, p2)):
        return x, y
    two, three, six, one = t(2), t(3), t(6), t(1)
    for _ in range(steps):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        drad = k1 + r2 * (two * k2 + r2 * (three * k3))
        ex = ((x * rad + (two * p1) * xy) + p2 * (r2 + two * xx)) - xd
        ey = ((y * rad + (two * p2) * xy) + p1 * (r2 + two * yy)) - yd
        jxx = ((rad + (two * xx) * drad) + (two * p1) * y) + (six * p2) * x
        jyy = ((rad + (two * yy) * drad) + (two * p2) * x) + (six * p1) * y
        jxy = ((two * xy) * drad + (two * p1) * x) + (two * p2) * y
        det = jxx * jyy - jxy * jxy
        ok = np.abs(det) >= t(DET_EPS)
        safe = np.where(ok, det, one)
        dx, dy = (jyy * ex - jxy * ey) / safe, (jxx * ey - jxy * ex) / safe
        x, y = np.where(ok, x - dx, x), np.where(ok, y - dy, y)
        if last is not None:
            last[:] = [float(np.max(np.abs(np.where(ok, dx, 0)))), float(np.max(np.abs(np.where(ok, dy, 0))))]
    return x, y


def rays(pose, row, cols, rows):
    """fp64 rays (n, 6) = [pose[:,3] | R.(xu, -yu, -1)] of the pixels, pose (3,4) taken in fp32 like the kernel's"""
    p = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(3, 4)
    xd, yd = pixel_plane(row, cols, rows)
    xu, yu = undistort(row, xd, yd)
    c = np.stack((xu, -yu, -np.ones_like(xu)), -1)
    return np.concatenate((np.broadcast_to(p[:, 3], c.shape), c @ p[:, :3].T), -1)


def kernel_model(pose, row, cols, rows, steps=NEWTON_STEPS, half=True, flip=True, drop_k3=False, swap_p=False, cx=None):
    """The kernels' rays in their own fp32 arithmetic, on the host (n, 6) fp32 -- and, through the keywords, with one fault planted:
    `half=False` drops the + 0.5, `flip=False` leaves y un-flipped, `cx` overrides the principal point's column, `steps`, `drop_k3`,
    `swap_p` as in undistort."""
    f = np.float32
    r = row.astype(f)
    p = np.asarray(pose, dtype=f).reshape(3, 4)
    hh = f(0.5) if half else f(0.0)
    xd = ((np.asarray(cols).astype(f) + hh) - (r[2] if cx is None else f(cx))) / r[0]
    yd = ((np.asarray(rows).astype(f) + hh) - r[3]) / r[1]
    x, y = undistort(r, xd, yd, steps=steps, dtype=f, drop_k3=drop_k3, swap_p=swap_p)
    cy = -y if flip else y
    d = [(x * p[i, 0] + cy * p[i, 1]) + f(-1.0) * p[i, 2] for i in range(3)]
    return np.stack([np.broadcast_to(p[i, 3], x.shape) for i in range(3)] + d, -1).astype(f)


def second_derivative_bound(row, R):
    k1, k2, k3, p1, p2 = np.abs(row[4:9])
    return 4.0 * (6.0 * k1 * R + 20.0 * k2 * R ** 3 + 42.0 * k3 * R ** 5 + 6.0 * (p1 + p2))


def backward_bound(row, cols, rows, xu, yu):
    """(Bx, By): the bound (1) on |F64(xu, yu) - (xd, yd)| per component, (xu, yu) the fp32 point a kernel returned"""
    xu, yu = np.asarray(xu, np.float64), np.asarray(yu, np.float64)
    if not np.any(row[4:9] != 0.0):                                 # no iteration: the point IS the fp32 pixel point, term (e) alone
        xd, yd = pixel_plane(row, cols, rows)
        xdh, ydh = pixel_plane32(row, cols, rows)
        return np.abs(xdh - xd), np.abs(ydh - yd)
    k1, k2, k3, p1, p2 = row[4:9]
    x, y = _Run(xu), _Run(yu)
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = _Run(1.0) + r2 * (_Run(k1) + r2 * (_Run(k2) + r2 * k3))
    xdh, ydh = pixel_plane32(row, cols, rows)
    ex = ((x * rad + _Run(2.0 * p1) * xy) + _Run(p2) * (r2 + xx.twice())) - xdh
    ey = ((y * rad + _Run(2.0 * p2) * xy) + _Run(p1) * (r2 + yy.twice())) - ydh
    a = (1.0 + 2.0 ** -8)
    jxx, jxy, jyy = (np.abs(j) for j in jacobian(row, xu, yu))
    c = jxx * h(xu) + jxy * h(yu), jxy * h(xu) + jyy * h(yu)
    R = float(max(np.max(np.abs(xu)), np.max(np.abs(yu)), 1e-30))
    bd = 64.0 * U * DELTA_LAST + second_derivative_bound(row, R) * DELTA_LAST ** 2
    xd, yd = pixel_plane(row, cols, rows)
    return a * ex.e + c[0] + bd + np.abs(xdh - xd), a * ey.e + c[1] + bd + np.abs(ydh - yd)


def backward_ratio(row, cols, rows, xu, yu):
    """max err / tol of check (1) for the fp32 points (xu, yu) a kernel returned for the pixels"""
    xd, yd = pixel_plane(row, cols, rows)
    fx, fy = distort(row, np.asarray(xu, np.float64), np.asarray(yu, np.float64))
    bx, by = backward_bound(row, cols, rows, xu, yu)
    tiny = 2.0 ** -149
    return float(max(np.max(np.abs(fx - xd) / np.maximum(bx, tiny)), np.max(np.abs(fy - yd) / np.maximum(by, tiny))))


def direction_ratio(pose, row, cols, rows, d):
    """max err / tol of check (2): d (n, 3) fp32 from a kernel against the fp64 rays, bound derived at the fp64 root"""
    p = np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(3, 4)
    xd, yd = pixel_plane(row, cols, rows)
    xs, ys = undistort(row, xd, yd)
    bx, by = backward_bound(row, cols, rows, xs.astype(np.float32), ys.astype(np.float32))
    jxx, jxy, jyy = jacobian(row, xs, ys)
    det = jxx * jyy - jxy * jxy
    a = (1.0 + 2.0 ** -8)
    dx = a * (np.abs(jyy) * bx + np.abs(jxy) * by) / np.abs(det)
    dy = a * (np.abs(jxy) * bx + np.abs(jxx) * by) / np.abs(det)
    want = np.stack((xs, -ys, -np.ones_like(xs)), -1) @ p[:, :3].T
    worst = 0.0
    for i in range(3):
        di = (_Run(xs, dx) * p[i, 0] + _Run(-ys, dy) * p[i, 1]) + _Run(-p[i, 2])
        worst = max(worst, float(np.max(np.abs(np.asarray(d, np.float64)[:, i] - want[:, i]) / np.maximum(di.e, 2.0 ** -149))))
    return worst


def grid(H, W):
    """(cols, rows) of every pixel in raster order"""
    rows, cols = np.divmod(np.arange(H * W), W)
    return cols, rows


# ------------------------------------------------------------------------------------------------ the test cameras
def cameras(H=33, W=47):
    """name -> camera row (fp64 values of the fp32 row) for an H x W image: an off-centre pinhole (cx = 20.25, cy = 18.75 at 33 x 47), the
    strong OPENCV camera (k1 = -0.12, k2 = 0.03, k3 = -0.004, p1 = 0.002, p2 = -0.0015) with the focal length that puts the farthest
    image corner just inside distorted radius 0.9, and a pure SIMPLE_RADIAL one (corner at 0.8)"""
    def focal_for(cx, cy, r):
        return float(np.hypot(max(cx - 0.5, W - 0.5 - cx), max(cy - 0.5, H - 0.5 - cy)) / r)
    out = {}
    out["pinhole"] = [40.0, 41.5, W / 2.0 - 3.25, H / 2.0 + 2.25, 0, 0, 0, 0, 0, 0, 0, 0]
    cx, cy = W / 2.0 + 0.625, H / 2.0 - 0.625
    fo = focal_for(cx, cy, 0.899)
    out["opencv"] = [fo, fo * 1.03125, cx, cy, -0.12, 0.03, -0.004, 0.002, -0.0015, 0, 0, 0]
    cx, cy = W / 2.0 - 0.5, H / 2.0 + 0.5
    fr = focal_for(cx, cy, 0.799)
    out["simple_radial"] = [fr, fr, cx, cy, -0.08, 0, 0, 0, 0, 0, 0, 0]
    return {k: np.asarray(v, dtype=np.float32).astype(np.float64) for k, v in out.items()}


def admit(row, H, W):
    """The conditions under which the fixed steps and the bounds hold, asserted over every pixel of an H x W image: det J > 0.3 at the
    start and at the root, distorted radius <= 0.9, fp64 residual after NEWTON_STEPS < 1e-12, last fp32 correction <= DELTA_LAST."""
    cols, rows = grid(H, W)
    xd, yd = pixel_plane(row, cols, rows)
    assert float(np.hypot(xd, yd).max()) <= 0.9
    xs, ys = undistort(row, xd, yd)
    for x, y in ((xd, yd), (xs, ys)):
        jxx, jxy, jyy = jacobian(row, x, y)
        assert float((jxx * jyy - jxy * jxy).min()) > 0.3
    fx, fy = distort(row, xs, ys)
    assert float(np.hypot(fx - xd, fy - yd).max()) < 1e-12
    if np.any(row[4:9] != 0.0):
        last = []
        xdh, ydh = pixel_plane32(row, cols, rows)
        undistort(row, xdh, ydh, dtype=np.float32, last=last)
        assert len(last) == 2 and max(last) <= DELTA_LAST


def camera_of(row):
    from nerf_amd.camera import Camera
    return Camera(*[float(v) for v in row[:9]])
