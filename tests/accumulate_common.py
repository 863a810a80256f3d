"""The numpy oracle of progressive multi-sample frames (include/stnerf.h: stnerf_generate_rays_list,
stnerf_accumulate, stnerf_accumulate_select): the pass schedule in fp64, rounded to fp32; the ray generator's operation order,
Welford's update and the select rule in fp32 throughout, ONE operation per line, so that numpy rounds after every operation as
the kernels (built without contraction) do.  Restated from the definitions, not from the package: nothing here imports it."""
from fractions import Fraction

import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------- schedule (fp64 -> fp32)
def radical_inverse(p, base):
    r = 0.0
    f = 1.0 / base
    while p:
        digit = p % base
        p = p // base
        r = r + digit * f
        f = f / base
    return r


def pass_schedule(p):
    """(du, dv, dt) of pass p: ((phi_b(p) + 0.5) mod 1) - 0.5, b = 2, 3, 5, as fp32 numbers."""
    out = []
    for base in (2, 3, 5):
        x = radical_inverse(p, base) + 0.5
        x = x - np.floor(x)
        x = x - 0.5
        out.append(F(x))
    return tuple(out)


def offset(p, pixel_filter=1.0):
    du, dv, _ = pass_schedule(p)
    return F(float(pixel_filter) * float(du)), F(float(pixel_filter) * float(dv))


def layer_frame_ids(p, frame_ids, shutters, frame_range=None):
    """f_i + shutter_i * dt_p in fp64, clamped, as fp32 numbers."""
    dt = float(pass_schedule(p)[2])
    out = []
    for f, s in zip(frame_ids, shutters):
        x = float(f) + float(s) * dt
        if frame_range is not None:
            x = min(max(x, float(frame_range[0])), float(frame_range[1]))
        out.append(F(x))
    return out


# ---------------------------------------------------------------------------------------- rays of a pixel list (fp32)
def _nearest_f32(x, candidates):
    """The fp32 number nearest to the exact rational x among neighbouring fp32 candidates, ties to the even mantissa."""
    best = min(candidates, key=lambda c: (abs(Fraction(float(c)) - x), int(np.asarray(c, F).view(np.uint32)) & 1))
    return F(best)


def fma32(a, b, c):
    """fmaf(a, b, c) on fp32 arrays: a b + c rounded ONCE to fp32.  The float64 product of two fp32 numbers is exact; the float64 sum
    rounds once to 53 bits, and rounding that again to 24 bits gives the wrong neighbour only where the float64 sum sits exactly
    halfway between two fp32 numbers -- those elements are decided in exact rational arithmetic."""
    a, b, c = (np.asarray(x, F) for x in np.broadcast_arrays(a, b, c))
    s = a.astype(np.float64) * b.astype(np.float64)
    s = s + c.astype(np.float64)
    r = s.astype(F)
    lo, hi = np.nextafter(r, F(-np.inf)), np.nextafter(r, F(np.inf))
    half_lo = (r.astype(np.float64) + lo.astype(np.float64)) / 2.0        # midpoints of neighbouring fp32 numbers: exact in float64
    half_hi = (r.astype(np.float64) + hi.astype(np.float64)) / 2.0
    tie = np.isfinite(s) & ((s == half_lo) | (s == half_hi))
    if tie.any():
        r = r.copy()
        for idx in zip(*np.nonzero(tie)):
            exact = Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx]))
            r[idx] = _nearest_f32(exact, (lo[idx], r[idx], hi[idx]))
    return r


def rays_of_pixels(kinv, T, w, pixels, du, dv, frame_ids=()):
    """generate_rays_kernel's operation order with u = (float)(pix % w) + du, v = (float)(pix / w) + dv; the squared norm is
    fmaf(z, z, fmaf(y, y, x x)) as there (torch.norm's order).  kinv (3,3), T (4,4) fp32."""
    kinv, T = np.asarray(kinv, F).reshape(9), np.asarray(T, F).reshape(16)
    pix = np.asarray(pixels, np.int64)
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
        xx = cam[0] * cam[0]
        s = fma32(cam[1], cam[1], xx)
        s = fma32(cam[2], cam[2], s)
        nrm = np.sqrt(s)
        cx = cam[0] / nrm
        cy = cam[1] / nrm
        cz = cam[2] / nrm
        out = np.empty((pix.shape[0], 6 + len(frame_ids)), F)
        out[:, 0], out[:, 1], out[:, 2] = T[3], T[7], T[11]
        for r in range(3):
            a = T[4 * r] * cx
            b = T[4 * r + 1] * cy
            c = T[4 * r + 2] * cz
            ab = a + b
            out[:, 3 + r] = ab + c
    for j, f in enumerate(frame_ids):
        out[:, 6 + j] = F(f)
    return out


# ---------------------------------------------------------------------------------------- Welford's update (fp32)
class State:
    def __init__(self, P, C, V=3):
        self.mean, self.m2, self.count = np.zeros((P, C), F), np.zeros((P, V), F), np.zeros(P, np.int32)

    def copy(self):
        s = State(1, 1, 1)
        s.mean, s.m2, s.count = self.mean.copy(), self.m2.copy(), self.count.copy()
        return s


def update(state, values, pixels=None):
    """One more sample (values (n,C) fp32) of the pixels ``pixels`` (None: pixels 0..n-1), in place."""
    x = np.asarray(values, F)
    n, V = x.shape[0], state.m2.shape[1]
    q = np.arange(n) if pixels is None else np.asarray(pixels, np.int64)
    assert len(set(q.tolist())) == n, "a list must not name a pixel twice"
    c = state.count[q] + np.int32(1)
    first = (c == 1)[:, None]
    with np.errstate(all="ignore"):
        m = state.mean[q]
        d = x - m
        step = d / c.astype(F)[:, None]
        mn = m + step
        back = x - mn
        prod = d * back
        m2n = state.m2[q] + prod[:, :V]
    state.mean[q] = np.where(first, x, mn)
    state.m2[q] = np.where(first, F(0), m2n)
    state.count[q] = c
    return state


# ---------------------------------------------------------------------------------------- the select rule (fp32)
def tol_squared(tol):
    t = F(tol)
    return t * t


def active(state, min_spp, max_spp, tol):
    c = state.count
    pairs = c * (c - np.int32(1))                     # the int32 product
    with np.errstate(all="ignore"):
        bound = tol_squared(tol) * pairs.astype(F)
        noisy = (state.m2 > bound[:, None]).any(1)
    return (c < min_spp) | ((c < max_spp) & noisy)


def select(state, min_spp, max_spp, tol):
    return np.flatnonzero(active(state, min_spp, max_spp, tol)).astype(np.int32)


def variance_of_mean(state):
    """m2 / (c (c - 1)), 0 where c < 2 (fp32)."""
    c = state.count.astype(F)[:, None]
    cm = c - F(1)
    den = c * cm
    with np.errstate(all="ignore"):
        out = state.m2 / np.maximum(den, F(1))
    return np.where(c >= 2, out, F(0)).astype(F)


def same_bits(a, b):
    """The same fp32 bits, a NaN matching any NaN (the payload of a NaN an operation produces is the hardware's own)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
