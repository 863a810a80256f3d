"""The numpy oracle of the lens model in ray generation (include/stnerf.h: stnerf_lens,
stnerf_generate_rays_lens): the per-row arithmetic in fp32, ONE operation per line, so that numpy rounds after every operation as
the kernel (built without contraction) does, the hash in uint32; the lens points of the passes and the Brown-Conrady forward model
in fp64.  Restated from the definitions, not from the package: nothing here imports it."""
import math

import numpy as np

from accumulate_common import fma32, same_bits  # noqa: F401  (fmaf on fp32 arrays; the bit comparison)

F = np.float32
ITERS = 20
SETS = ((-0.1, 0.02, 0.0, 0.001, -0.0005), (-0.28, 0.09, -0.01, 0.002, 0.001), (0.2, 0.05, 0.0, 0.0, 0.0), (-0.35, 0.15, -0.03, 0.0, 0.0))


# ---------------------------------------------------------------------------------------- the lens points (fp64 -> fp32)
def lens_point(p):
    """The unit-disk point of pass p: the R2 sequence on the square, the Shirley-Chiu concentric map, rounded to fp32."""
    a = 0.5 + p * 0.7548776662466927
    a = a - math.floor(a)
    a = a * 2.0 - 1.0
    b = 0.5 + p * 0.5698402909980532
    b = b - math.floor(b)
    b = b * 2.0 - 1.0
    if a == 0.0 and b == 0.0:
        return F(0.0), F(0.0)
    if abs(a) > abs(b):
        r = a
        theta = (math.pi / 4.0) * (b / a)
    else:
        r = b
        theta = math.pi / 2.0 - (math.pi / 4.0) * (a / b)
    return F(r * math.cos(theta)), F(r * math.sin(theta))


def table(n, aperture):
    """(n, 2) fp32: lens_point(p) times the aperture, each product rounded once."""
    out = np.empty((n, 2), F)
    for p in range(n):
        x, y = lens_point(p)
        out[p, 0] = F(float(aperture) * float(x))
        out[p, 1] = F(float(aperture) * float(y))
    return out


# ---------------------------------------------------------------------------------------- distortion (fp64 forward model)
def forward64(x, y, k1, k2, k3, p1, p2):
    """Brown-Conrady, the OpenCV order: undistorted normalised (x, y) -> distorted, in fp64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    tx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    ty = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return x * rad + tx, y * rad + ty


# ---------------------------------------------------------------------------------------- the hash and the walk (uint32)
def lens_hash(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def table_rows(pixels, n_points, phase, decorrelate, key=0):
    """The table row every pixel uses in pass ``phase``."""
    pix = np.asarray(pixels, np.int64)
    if not decorrelate:
        return np.full(pix.shape, phase, np.int64)
    with np.errstate(over="ignore"):
        hsh = lens_hash(pix.astype(np.uint32) ^ np.uint32(key))
    start = hsh % np.uint32(n_points)
    j = start + np.uint32(phase)
    j = j % np.uint32(n_points)
    return j.astype(np.int64)


# ---------------------------------------------------------------------------------------- the rays (fp32)
def rays_of_lens(kinv, T, w, pixels, du=0.0, dv=0.0, frame_ids=(), coeffs=None, points=None, phase=0, decorrelate=False, key=0, focus=0.0):
    """generate_rays_lens_kernel's operation order.  kinv (3,3), T (4,4) fp32; coeffs = (k1, k2, k3, p1, p2) or None: no distortion;
    points (n_points, 2) fp32 or None: pinhole."""
    kinv, T = np.asarray(kinv, F).reshape(9), np.asarray(T, F).reshape(16)
    pix = np.asarray(pixels, np.int64)
    n = pix.shape[0]
    with np.errstate(all="ignore"):
        u = (pix % w).astype(F)
        u = u + F(du)
        v = (pix // w).astype(F)
        v = v + F(dv)
        cam = []
        for r in range(3):
            a = kinv[3 * r] * u
            b = kinv[3 * r + 1] * v
            ab = a + b
            cam.append(ab + kinv[3 * r + 2])
        cx, cy, cz = cam
        if coeffs is not None:
            k1, k2, k3, p1, p2 = (F(c) for c in coeffs)
            xd = cx / cz
            yd = cy / cz
            x, y = xd, yd
            for _ in range(ITERS):
                xx = x * x
                yy = y * y
                xy = x * y
                r2 = xx + yy
                rad = k3 * r2
                rad = rad + k2
                rad = rad * r2
                rad = rad + k1
                rad = rad * r2
                rad = rad + F(1.0)
                xy2 = xy + xy
                xx2 = xx + xx
                yy2 = yy + yy
                ta = p1 * xy2
                tb = r2 + xx2
                tb = p2 * tb
                tx = ta + tb
                tc = r2 + yy2
                tc = p1 * tc
                td = p2 * xy2
                ty = tc + td
                x = xd - tx
                x = x / rad
                y = yd - ty
                y = y / rad
            cx = x * cz
            cy = y * cz
        o = [np.full(n, T[3], F), np.full(n, T[7], F), np.full(n, T[11], F)]
        if points is not None:
            points = np.asarray(points, F)
            j = table_rows(pix, points.shape[0], phase, decorrelate, key)
            ax, ay = points[j, 0], points[j, 1]
            thin = ~((ax == 0) & (ay == 0))
            s = F(focus) / cz
            dx = cx * s
            dx = dx - ax
            dy = cy * s
            dy = dy - ay
            dz = cz * s
            cx, cy, cz = np.where(thin, dx, cx), np.where(thin, dy, cy), np.where(thin, dz, cz)
            for r in range(3):
                a = T[4 * r] * ax
                b = T[4 * r + 1] * ay
                ab = a + b
                ab = ab + T[4 * r + 3]
                o[r] = np.where(thin, ab, o[r])
        xx = cx * cx
        s2 = fma32(cy, cy, xx)
        s2 = fma32(cz, cz, s2)
        nrm = np.sqrt(s2)
        cx = cx / nrm
        cy = cy / nrm
        cz = cz / nrm
        out = np.empty((n, 6 + len(frame_ids)), F)
        out[:, 0], out[:, 1], out[:, 2] = o
        for r in range(3):
            a = T[4 * r] * cx
            b = T[4 * r + 1] * cy
            c = T[4 * r + 2] * cz
            ab = a + b
            out[:, 3 + r] = ab + c
    for k, f in enumerate(frame_ids):
        out[:, 6 + k] = F(f)
    return out


def intrinsics(f, h, w):
    """K of focal length f (pixels) with the principal point at the view's centre, and its fp32 inverse as torch.inverse gives it."""
    import torch
    K = torch.tensor([[f, 0.0, 0.5 * (w - 1)], [0.0, f, 0.5 * (h - 1)], [0.0, 0.0, 1.0]], dtype=torch.float32)
    return K, torch.inverse(K).numpy()
