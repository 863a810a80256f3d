"""A lens model for ray generation: distortion and depth of field.

Both are properties of the camera and live in one place, the ray generator (``ops.generate_rays(lens=)``,
csrc/lens.hip): a distorting lens bends the ray of a pixel (Brown-Conrady, inverted by a fixed number of fixed-point rounds), a
lens with an aperture starts it at a point of the lens and sends it through the pinhole ray's point on the plane in focus.  The
points of the lens are a low-discrepancy sequence on the unit disk, one per pass of an accumulated frame
(``parallel.render_view_accumulated``).  This module is the host arithmetic, which is exact and needs no GPU.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

ITERS = 20                      # (STNERF_LENS_ITERS: the rounds of the fixed-point inverse)
R2_A = 0.7548776662466927       # the R2 sequence's two constants: 1 / g and 1 / g^2, g the plastic number
R2_B = 0.5698402909980532
CHECK_TOL = 1e-6                # residual of the forward model after ITERS rounds, normalised units (``Lens.check``)


def lens_point(p: int) -> Tuple[float, float]:
    """The unit-disk point of pass p >= 0, computed in fp64 and rounded to fp32: the R2 sequence
    (a, b) = ((0.5 + p R2_A) mod 1, (0.5 + p R2_B) mod 1) * 2 - 1 on the square, mapped to the disk by the Shirley-Chiu
    concentric map ((0, 0) -> (0, 0); |a| > |b|: r = a, theta = (pi/4)(b/a); else r = b, theta = pi/2 - (pi/4)(a/b)).
    Pass 0 is the lens centre, so the first pass of a frame is the pinhole render."""
    if int(p) != p or p < 0:
        raise ValueError(f"lens_point: the pass is a whole number >= 0, got {p!r}")
    p = int(p)
    a = math.fmod(0.5 + p * R2_A, 1.0) * 2.0 - 1.0
    b = math.fmod(0.5 + p * R2_B, 1.0) * 2.0 - 1.0
    if a == 0.0 and b == 0.0:
        return 0.0, 0.0
    if abs(a) > abs(b):
        r, theta = a, (math.pi / 4.0) * (b / a)
    else:
        r, theta = b, math.pi / 2.0 - (math.pi / 4.0) * (a / b)
    return float(np.float32(r * math.cos(theta))), float(np.float32(r * math.sin(theta)))


def forward_distortion(x, y, k1, k2, k3, p1, p2):
    """The Brown-Conrady forward model (the OpenCV order) on normalised image coordinates, in the dtype of its inputs:
    undistorted (x, y) -> distorted."""
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0
    tx = p1 * (xy + xy) + p2 * (r2 + (xx + xx))
    ty = p1 * (r2 + (yy + yy)) + p2 * (xy + xy)
    return x * rad + tx, y * rad + ty


def _finite32(x: float) -> bool:
    """Is x finite as the fp32 number the library gets?"""
    with np.errstate(over="ignore"):
        return bool(np.isfinite(x) and np.isfinite(np.float32(x)))


def _kinv(K) -> np.ndarray:
    """K^-1 as the ray generator gets it (torch.inverse of the fp32 K on the host), as fp64 numbers."""
    import torch
    return torch.inverse(torch.as_tensor(K).detach().to("cpu", torch.float32)).numpy().astype(np.float64)


class Lens:
    """A camera's lens.

    k1, k2, k3, p1, p2   Brown-Conrady distortion coefficients (the OpenCV order) on normalised image coordinates; all zero: none.
    aperture             the lens radius in world units (>= 0; 0: a pinhole, no defocus).
    focus                distance to the plane in focus along the optical axis (world units); required and > 0 with aperture > 0.
    decorrelate          every pixel walks the table of lens points from its own start (default True: the passes of neighbouring
                         pixels use different points, so defocus shows as noise that averages out, not as shifted copies).
    key                  a 32-bit number xor-ed into the pixel before hashing: another decorrelation pattern.
    """

    def __init__(self, k1: float = 0.0, k2: float = 0.0, k3: float = 0.0, p1: float = 0.0, p2: float = 0.0, aperture: float = 0.0,
                 focus: Optional[float] = None, decorrelate: bool = True, key: int = 0):
        self.k1, self.k2, self.k3, self.p1, self.p2 = (float(x) for x in (k1, k2, k3, p1, p2))
        if not all(_finite32(x) for x in self.coefficients):
            raise ValueError(f"Lens: the distortion coefficients must be finite, got {self.coefficients!r}")
        self.aperture = float(aperture)
        if not (self.aperture >= 0.0 and _finite32(self.aperture)):
            raise ValueError(f"Lens: aperture (the lens radius) must be >= 0 and finite, got {aperture!r}")
        self.focus = None if focus is None else float(focus)
        if self.focus is not None and not (_finite32(self.focus) and float(np.float32(self.focus)) > 0.0):
            raise ValueError(f"Lens: focus (the distance to the plane in focus) must be > 0 and finite, got {focus!r}")
        if self.aperture > 0.0 and self.focus is None:
            raise ValueError("Lens: aperture > 0 needs focus=, the distance to the plane in focus")
        self.decorrelate = bool(decorrelate)
        if int(key) != key or not 0 <= int(key) < (1 << 32):
            raise ValueError(f"Lens: key is a 32-bit unsigned number, got {key!r}")
        self.key = int(key)

    def __repr__(self):
        return (f"Lens(k1={self.k1}, k2={self.k2}, k3={self.k3}, p1={self.p1}, p2={self.p2}, aperture={self.aperture}, focus={self.focus}, "
                f"decorrelate={self.decorrelate}, key={self.key})")

    @property
    def coefficients(self) -> Tuple[float, float, float, float, float]:
        return self.k1, self.k2, self.k3, self.p1, self.p2

    @property
    def distorts(self) -> bool:
        return any(c != 0.0 for c in self.coefficients)

    @property
    def enabled(self) -> bool:
        """False: the pinhole camera -- every call then launches exactly what it launches without a lens."""
        return self.distorts or self.aperture > 0.0

    def table(self, n: int) -> np.ndarray:
        """(n, 2) fp32: the lens points of passes 0..n-1 in camera x, y, world units -- ``lens_point(p)`` times ``aperture``, each
        product rounded to fp32 once.  Uploaded once per frame."""
        if int(n) != n or n < 1:
            raise ValueError(f"Lens.table: need n >= 1 points, got {n!r}")
        out = np.empty((int(n), 2), np.float32)
        for p in range(int(n)):
            x, y = lens_point(p)
            out[p, 0] = np.float32(self.aperture * x)
            out[p, 1] = np.float32(self.aperture * y)
        return out

    def undistort(self, xd, yd):
        """The ITERS rounds of the ray generator's fixed-point inverse in fp64: distorted normalised coordinates -> undistorted."""
        xd, yd = np.asarray(xd, np.float64), np.asarray(yd, np.float64)
        x, y = xd, yd
        with np.errstate(all="ignore"):
            for _ in range(ITERS):
                xx, yy, xy = x * x, y * y, x * y
                r2 = xx + yy
                rad = ((self.k3 * r2 + self.k2) * r2 + self.k1) * r2 + 1.0
                tx = self.p1 * (xy + xy) + self.p2 * (r2 + (xx + xx))
                ty = self.p1 * (r2 + (yy + yy)) + self.p2 * (xy + xy)
                x, y = (xd - tx) / rad, (yd - ty) / rad
        return x, y

    def check(self, K, h: int, w: int) -> None:
        """Is this lens usable with the view (K, h, w)?  In fp64: K^-1's third row must be (0, 0, k), k != 0 (the plane in focus
        and the division by the camera vector's z assume one z for the view), and the fixed-point inverse must have converged at
        the view's four corners and four edge midpoints -- the residual of the forward model there is at most 1e-6 in normalised
        units.  ValueError otherwise: a lens too strong for ITERS rounds at this field of view."""
        kinv = _kinv(K)
        if not (kinv[2, 0] == 0.0 and kinv[2, 1] == 0.0 and kinv[2, 2] != 0.0 and np.isfinite(kinv[2, 2])):
            raise ValueError(f"Lens.check: the third row of K^-1 must be (0, 0, k) with k != 0, got {kinv[2].tolist()}: a lens assumes "
                             "one camera-space z for the view")
        if not self.distorts:
            return
        us, vs = (0.0, 0.5 * (w - 1), float(w - 1)), (0.0, 0.5 * (h - 1), float(h - 1))
        uv = np.array([(u, v, 1.0) for j, v in enumerate(vs) for i, u in enumerate(us) if (i, j) != (1, 1)])
        cam = uv @ kinv.T
        xd, yd = cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2]
        x, y = self.undistort(xd, yd)
        with np.errstate(all="ignore"):
            fx, fy = forward_distortion(x, y, *self.coefficients)
            res = np.maximum(np.abs(fx - xd), np.abs(fy - yd))
        if not np.all(np.isfinite(res)) or float(res.max()) > CHECK_TOL:
            raise ValueError(f"Lens.check: the lens is too strong for the {ITERS}-round fixed-point inverse at this field of view "
                             f"({h} x {w}): the residual of the forward model at the view's border is {float(np.nanmax(res)):.3e} in "
                             f"normalised units (at most {CHECK_TOL:g})")

    def fingerprint(self) -> tuple:
        """Every field, as a hashable tuple: what joins the view key of the background and layer caches, so that they miss when
        the lens changes at the same K, T."""
        return (self.k1, self.k2, self.k3, self.p1, self.p2, self.aperture, self.focus, self.decorrelate, self.key)


def as_lens(lens) -> Optional[Lens]:
    """A ``Lens`` from one, from the dict of its arguments, or None."""
    if lens is None or isinstance(lens, Lens):
        return lens
    if isinstance(lens, dict):
        return Lens(**lens)
    raise TypeError(f"lens is a Lens or the dict of its arguments, got {type(lens).__name__}")


def enabled(lens) -> bool:
    """True when ``lens`` (None | Lens) changes any ray."""
    return lens is not None and lens.enabled
