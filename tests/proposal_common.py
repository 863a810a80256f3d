"""Shared by tests/test_gpu_proposal.py and tests/test_proposal_cpu.py: the numpy restatement of the grid proposals' lookup
(include/stnerf.h: stnerf_density_grid), one fp32 operation per line, its fp64 counterpart, and the hand-made
grids and points of the kernel tests."""
import numpy as np

F = np.float32
U = 2.0 ** -24                     # half an ulp of 1: the relative rounding error of one fp32 operation
NAN = F(np.nan)


def np_axis(p, lo, inv, r):
    """One axis of the lookup: p fp32 array -> (i int32, f, u fp32), every line one fp32 operation."""
    p = np.asarray(p, F)
    with np.errstate(all="ignore"):
        d = p - F(lo)
        g = d * F(inv)
        gc = np.fmin(np.fmax(g, F(0)), F(r))          # (fmaxf / fminf: a NaN operand is dropped)
        i = np.fmin(np.floor(gc), F(r - 1)).astype(np.int32)
        f = gc - i.astype(F)
        u = F(1) - f
    assert d.dtype == g.dtype == gc.dtype == f.dtype == u.dtype == F
    return i, f, u


def np_lerp(v0, u, v1, f):
    with np.errstate(all="ignore"):
        a = v0 * u
        b = v1 * f
        return a + b


def np_lookup(xyz, sigma, lo, inv):
    """xyz (..., 3) fp32, sigma [Rz+1][Ry+1][Rx+1] fp32, lo / inv (3,) fp32 -> sigma at the points, fp32 (...)."""
    xyz, sigma = np.asarray(xyz, F), np.asarray(sigma, F)
    rz, ry, rx = (s - 1 for s in sigma.shape)
    ix, fx, ux = np_axis(xyz[..., 0], lo[0], inv[0], rx)
    iy, fy, uy = np_axis(xyz[..., 1], lo[1], inv[1], ry)
    iz, fz, uz = np_axis(xyz[..., 2], lo[2], inv[2], rz)
    v = lambda dz, dy, dx: sigma[iz + dz, iy + dy, ix + dx]
    c00 = np_lerp(v(0, 0, 0), ux, v(0, 0, 1), fx)
    c10 = np_lerp(v(0, 1, 0), ux, v(0, 1, 1), fx)
    c01 = np_lerp(v(1, 0, 0), ux, v(1, 0, 1), fx)
    c11 = np_lerp(v(1, 1, 0), ux, v(1, 1, 1), fx)
    c0 = np_lerp(c00, uy, c10, fy)
    c1 = np_lerp(c01, uy, c11, fy)
    s = np_lerp(c0, uz, c1, fz)
    assert s.dtype == F
    return np.where(np.isnan(xyz).any(-1), NAN, s)


def np_proposal_raw(xyz, sigma, lo, inv):
    """The rows the kernel writes: (..., 4) = {0, 0, 0, sigma}."""
    s = np_lookup(xyz, sigma, lo, inv)
    return np.concatenate([np.zeros(s.shape + (3,), F), s[..., None]], -1)


def same_sigma(a, b):
    """Bit for bit, with any NaN equal to any NaN (the payload of a NaN an operation makes differs between processors)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def exact_lookup(xyz, sigma, lo, inv):
    """Trilinear interpolation in fp64 at fp64 points (the grid's fp32 numbers taken as they are); points clamp to the box."""
    xyz, sigma = np.asarray(xyz, np.float64), np.asarray(sigma, np.float64)
    rz, ry, rx = (s - 1 for s in sigma.shape)
    idx, frac = [], []
    for a, r in enumerate((rx, ry, rz)):
        g = np.clip((xyz[..., a] - float(lo[a])) * float(inv[a]), 0.0, float(r))
        i = np.minimum(np.floor(g), r - 1).astype(np.int64)
        idx.append(i)
        frac.append(g - i)
    (ix, iy, iz), (fx, fy, fz) = idx, frac
    out = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (fx if dx else 1 - fx) * (fy if dy else 1 - fy) * (fz if dz else 1 - fz)
                out = out + w * sigma[iz + dz, iy + dy, ix + dx]
    return out


def grid_of(res, seed, lo=(-1.25, 0.5, 2.0), extent=(1.7, 0.9, 2.3), infs=True):
    """A test grid: random vertex values in [0, 8) with a few +-inf -> (sigma [Rz+1][Ry+1][Rx+1], lo, hi, inv) in fp32."""
    g = np.random.default_rng(seed)
    rx, ry, rz = res
    sigma = (g.random((rz + 1, ry + 1, rx + 1)) * 8).astype(F)
    if infs:
        flat = sigma.reshape(-1)
        flat[g.integers(0, flat.size, max(1, flat.size // 40))] = np.inf
        flat[g.integers(0, flat.size, 1)] = -np.inf
    lo = np.asarray(lo, F)
    hi = (lo + np.asarray(extent, F)).astype(F)
    inv = (np.asarray(res, F) / (hi - lo)).astype(F)
    return sigma, lo, hi, inv


def special_points(lo, hi):
    """The points every kernel case must include: exactly lo, exactly hi, one ulp on either side of each, far outside, +-inf and a
    NaN per axis -> (m, 3) fp32."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    mid = ((lo + hi) / 2).astype(F)
    rows = [lo, hi, np.nextafter(lo, F(-np.inf)), np.nextafter(lo, F(np.inf)), np.nextafter(hi, F(-np.inf)), np.nextafter(hi, F(np.inf)),
            lo - F(1e6), hi + F(1e6), np.full(3, -np.inf, F), np.full(3, np.inf, F)]
    for a in range(3):
        for v in (lo[a], hi[a], np.nextafter(lo[a], F(-np.inf)), np.nextafter(hi[a], F(np.inf)), F(-1e30), F(1e30), F(-np.inf), F(np.inf), NAN):
            p = mid.copy()
            p[a] = v
            rows.append(p)
    return np.stack(rows).astype(F)


def points_of(n, ns, lo, hi, seed):
    """(n, ns, 3) fp32: random points in the box grown by a fifth on every side, the special points spread over the first samples."""
    g = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    ext = hi - lo
    pts = (lo - F(0.2) * ext + g.random((n, ns, 3)).astype(F) * (F(1.4) * ext)).astype(F)
    sp = special_points(lo, hi)
    flat = pts.reshape(-1, 3)
    at = g.permutation(flat.shape[0])[:sp.shape[0]]
    flat[at] = sp[:len(at)]
    return pts, int(len(at))
