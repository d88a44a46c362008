"""The camera model of the ray-forming kernels (include/nerf_amd.h): focal lengths, principal point and OpenCV / COLMAP lens distortion,
one row of 12 fp32 values per camera.  ``render_image(camera=...)`` takes one, ``TrainStep(cameras=...)`` one per view."""
from typing import Sequence

import torch

ROW = 12                    # NERF_AMD_CAMERA_ROW: fx fy cx cy k1 k2 k3 p1 p2 + three reserved zeros

# COLMAP camera model -> the positions of its parameters in (fx, fy, cx, cy, k1, k2, k3, p1, p2); "f" fills fx and fy
_COLMAP = {
    "SIMPLE_PINHOLE": ("f", "cx", "cy"),
    "PINHOLE": ("fx", "fy", "cx", "cy"),
    "SIMPLE_RADIAL": ("f", "cx", "cy", "k1"),
    "RADIAL": ("f", "cx", "cy", "k1", "k2"),
    "OPENCV": ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"),
}


class Camera:
    """``cx, cy`` are in pixels in COLMAP's convention: the centre of pixel (col, row) is at (col + 0.5, row + 0.5).  The ray of a pixel
    is o = pose[:,3], d = R.(xu, -yu, -1) with (xu, yu) the undistorted image-plane point: the project's cameras look down -z with y up.
    COLMAP stores world-to-camera poses of cameras that look down +z with y down; converting such a pose to the (3,4) camera-to-world
    matrix used here is the caller's job."""

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, p1=0.0, p2=0.0):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.k1, self.k2, self.k3, self.p1, self.p2 = float(k1), float(k2), float(k3), float(p1), float(p2)
        vals = self.row()
        if not all(v == v and abs(v) != float("inf") for v in vals):
            raise ValueError("nerf_amd.Camera: every parameter must be finite")
        if not (self.fx > 0.0 and self.fy > 0.0):
            raise ValueError("nerf_amd.Camera: fx and fy must be positive")

    @classmethod
    def reference(cls, H: int, W: int, focal, sampler: bool = False) -> "Camera":
        """Today's camera as a row: the pinhole whose rays ``ops.generate_rays`` forms (cx = W/2, cy = H/2 + 1: that table adds its 0.5
        after the y flip), or with ``sampler=True`` the training samplers' (integer halves: cx = W//2, cy = H//2 + 1).  ``focal``: a
        scalar, or (fy, fx) like everywhere in the package.  The kernels reproduce those rays bit for bit."""
        from .utils import _focal_xy
        fx, fy = _focal_xy(focal)
        if sampler:
            return cls(fx, fy, int(W) // 2, int(H) // 2 + 1)
        return cls(fx, fy, int(W) / 2.0, int(H) / 2.0 + 1.0)

    @classmethod
    def from_colmap(cls, model: str, params: Sequence[float]) -> "Camera":
        """A camera of COLMAP's cameras.txt / cameras.bin: ``model`` one of SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV and
        ``params`` in COLMAP's order for it."""
        names = _COLMAP.get(str(model).upper())
        if names is None:
            raise ValueError("nerf_amd.Camera.from_colmap: camera model %r is not supported (supported: %s)" % (model, ", ".join(_COLMAP)))
        params = [float(p) for p in params]
        if len(params) != len(names):
            raise ValueError("nerf_amd.Camera.from_colmap: %s takes %d parameters (%s), got %d" % (model, len(names), ", ".join(names), len(params)))
        kw = dict(zip(names, params))
        if "f" in kw:
            kw["fx"] = kw["fy"] = kw.pop("f")
        return cls(**kw)

    def scaled(self, s: float) -> "Camera":
        """The camera of the image resized by the factor ``s``: fx, fy, cx, cy scale, the coefficients act on normalised coordinates and stay."""
        s = float(s)
        if not s > 0.0:
            raise ValueError("nerf_amd.Camera.scaled: the factor must be positive")
        return Camera(self.fx * s, self.fy * s, self.cx * s, self.cy * s, self.k1, self.k2, self.k3, self.p1, self.p2)

    def row(self) -> list:
        """The 12-value camera row (include/nerf_amd.h)."""
        return [self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.k3, self.p1, self.p2, 0.0, 0.0, 0.0]

    @staticmethod
    def table(cameras, device) -> torch.Tensor:
        """(V, 12) fp32 on ``device``: row v the camera of view v."""
        cameras = list(cameras)
        if not cameras or not all(isinstance(c, Camera) for c in cameras):
            raise ValueError("nerf_amd.Camera.table: needs a non-empty sequence of Camera")
        return torch.tensor([c.row() for c in cameras], dtype=torch.float32).to(device)

    def distort(self, x, y):
        """The forward model on normalised image-plane coordinates (tensors or floats): (x, y) -> (xd, yd); the pixel of a camera-space
        point (X, Y, Z), Z < 0, is col + 0.5 = fx xd + cx, row + 0.5 = fy yd + cy at (x, y) = (X / -Z, -Y / -Z)."""
        r2 = x * x + y * y
        rad = 1.0 + r2 * (self.k1 + r2 * (self.k2 + r2 * self.k3))
        xd = x * rad + 2.0 * self.p1 * x * y + self.p2 * (r2 + 2.0 * x * x)
        yd = y * rad + 2.0 * self.p2 * x * y + self.p1 * (r2 + 2.0 * y * y)
        return xd, yd

    def __repr__(self):
        return "Camera(fx=%r, fy=%r, cx=%r, cy=%r, k1=%r, k2=%r, k3=%r, p1=%r, p2=%r)" % tuple(self.row()[:9])
