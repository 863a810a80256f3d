"""The numpy oracle of reprojection into a nearby view (include/stnerf.h: stnerf_reproject_splat,
stnerf_reproject_resolve, stnerf_reproject_holes): splat, resolve and the hole list in fp32 throughout, ONE operation per line, so
that numpy rounds after every operation as the kernels (built without contraction) do; the minimum of a destination pixel is taken
by sorting the uint64 keys.  Restated from the definitions, not from the package: nothing here imports it.

Beside it an fp64 geometric check (``geometry_errors``) that shares no code with the restatement, the analytic source frame the
tests warp (a far plane z = 2 with a near strip z = 0 over the central third of x, ray parameters from the exact ray-plane
intersection, values a function of the world point), and the case set of the GPU tests."""
import numpy as np

from accumulate_common import F, fma32, rays_of_pixels, same_bits  # noqa: F401  (same_bits: for the tests)

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
H, W = 17, 23                     # the view of tests/scene_edits_common.py: 391 rays
C = 5
REL = 0.05                        # the tests' guard: t' may exceed the nearest neighbour's by 5 %
Z_MIN = 1e-6
POISON = 0x7fc0beef               # a NaN with a payload no operation produces (tests/test_gpu_accumulate.py)


# ---------------------------------------------------------------------------------------- cameras (fp64 -> fp32)
def camera(h, w, orbit_deg=0.0, dist=4.0, focal=None):
    """K = [[f,0,w/2],[0,f,h/2],[0,0,1]], f = w unless given; T = camera-to-world looking at the origin from ``dist`` on a circle in
    the x-z plane (orbit 0: at (0,0,-dist) looking down +z) -- the synthetic scenes' camera, as fp32 arrays."""
    f = float(w) if focal is None else float(focal)
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]], F)
    a = np.deg2rad(orbit_deg)
    c, s = float(np.cos(a)), float(np.sin(a))
    T = np.array([[c, 0.0, s, -dist * s], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, -dist * c], [0.0, 0.0, 0.0, 1.0]], F)
    return K, T


def kinv_of(K):
    """K^-1 as the ray generator's callers take it: torch.inverse of the fp32 matrix on the host."""
    import torch
    return torch.inverse(torch.from_numpy(np.asarray(K, F).reshape(3, 3).copy())).numpy().astype(F)


def world_to_camera(T):
    """Wd (3,4): the inverse of the pose in fp64, rounded once to fp32."""
    return np.linalg.inv(np.asarray(T, F).reshape(4, 4).astype(np.float64))[:3, :4].astype(F)


# ---------------------------------------------------------------------------------------- the analytic source frame (fp64)
def analytic_frame(K, T, h, w, n=None):
    """-> (t (n,) fp32, values (n,C) fp32) of the first n pixels of a view of the two-plane scene.  Everything in fp64 (its own
    ray: K^-1 by numpy, no fp32 step), rounded at the end; a ray that meets neither plane in front of it is absent (NaN)."""
    n = h * w if n is None else n
    q = np.arange(n)
    Ki = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
    Tm = np.asarray(T, np.float64).reshape(4, 4)
    cam = Ki @ np.stack([(q % w).astype(np.float64), (q // w).astype(np.float64), np.ones(n)])
    cam = cam / np.linalg.norm(cam, axis=0)
    d = (Tm[:3, :3] @ cam).T
    o = Tm[:3, 3]
    with np.errstate(all="ignore"):
        t_near = (0.0 - o[2]) / d[:, 2]
        t_far = (2.0 - o[2]) / d[:, 2]
    x_near = o[0] + t_near * d[:, 0]
    strip = (t_near > 0) & (np.abs(x_near) <= 2.0 / 3.0)
    t = np.where(strip, t_near, np.where(t_far > 0, t_far, np.nan))
    p = o[None, :] + t[:, None] * d
    with np.errstate(all="ignore"):
        values = np.stack([np.sin(3.0 * p[:, 0]), np.cos(2.0 * p[:, 1]), p[:, 2], p[:, 0] * p[:, 1], 0.25 + 0.0 * p[:, 0]], 1)
    values = np.where(np.isfinite(t)[:, None], values, 0.0)
    return t.astype(F), values.astype(F)


# ---------------------------------------------------------------------------------------- splat (fp32)
def splat_rows(kinv_s, T_s, w_s, t_src, id_base, K_d, Wd, o_d, h_d, w_d, z_min=Z_MIN):
    """The rows of one source that reach the destination -> (target pixel (m,) int64, key (m,) uint64), in row order."""
    K_d, Wd, o_d = np.asarray(K_d, F).reshape(9), np.asarray(Wd, F).reshape(12), np.asarray(o_d, F).reshape(3)
    t = np.asarray(t_src, F)
    n = t.shape[0]
    q = np.arange(n, dtype=np.int64)
    rays = rays_of_pixels(kinv_s, T_s, w_s, q, 0.0, 0.0)
    with np.errstate(all="ignore"):
        present = np.isfinite(t) & (t > F(0))
        p = []
        for r in range(3):
            a = t * rays[:, 3 + r]
            p.append(a + rays[:, r])
        c = []
        for r in range(3):
            a = Wd[4 * r] * p[0]
            b = Wd[4 * r + 1] * p[1]
            ab = a + b
            e = Wd[4 * r + 2] * p[2]
            abe = ab + e
            c.append(abe + Wd[4 * r + 3])
        keep = present & ~(c[2] <= F(z_min))
        pix = []
        for r in range(3):
            a = K_d[3 * r] * c[0]
            b = K_d[3 * r + 1] * c[1]
            ab = a + b
            e = K_d[3 * r + 2] * c[2]
            pix.append(ab + e)
        u = pix[0] / pix[2]
        v = pix[1] / pix[2]
        ru = np.rint(u)
        rv = np.rint(v)
        keep &= np.isfinite(u) & np.isfinite(v) & (ru >= 0) & (ru < w_d) & (rv >= 0) & (rv < h_d)
        e0 = p[0] - o_d[0]
        e1 = p[1] - o_d[1]
        e2 = p[2] - o_d[2]
        s = e0 * e0
        s = fma32(e1, e1, s)
        s = fma32(e2, e2, s)
        tp = np.sqrt(s).astype(F)
    iu = np.where(keep, ru, 0).astype(np.int64)
    iv = np.where(keep, rv, 0).astype(np.int64)
    ids = (np.int64(id_base) + q).astype(np.uint64)
    key = (tp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids
    return (iv * w_d + iu)[keep], key[keep]


def splat(sources, K_d, T_d, h_d, w_d, z_min=Z_MIN, id_bases=None):
    """sources: [(kinv, T, h, w, values, t)].  -> (keys (h_d w_d,) uint64, candidates): the per-pixel minimum, taken by SORTING
    the (target, key) pairs; candidates = {target: sorted list of every key that reached it} for the tests' case census."""
    Wd, o_d = world_to_camera(T_d), np.asarray(T_d, F).reshape(4, 4)[:3, 3]
    targets, keys = [], []
    base = 0
    for i, (kinv, T, h, w, values, t) in enumerate(sources):
        b = base if id_bases is None else id_bases[i]
        tg, ky = splat_rows(kinv, T, w, t, b, K_d, Wd, o_d, h_d, w_d, z_min)
        targets.append(tg)
        keys.append(ky)
        base += len(t)
    targets, keys = np.concatenate(targets), np.concatenate(keys)
    order = np.lexsort((keys, targets))               # by target, then by key: the first of a target is its minimum
    targets, keys = targets[order], keys[order]
    out = np.full(h_d * w_d, EMPTY, np.uint64)
    first = np.ones(len(targets), bool)
    first[1:] = targets[1:] != targets[:-1]
    out[targets[first]] = keys[first]
    candidates = {}
    for tg, ky in zip(targets.tolist(), keys.tolist()):
        candidates.setdefault(tg, []).append(ky)
    return out, candidates


# ---------------------------------------------------------------------------------------- resolve and the hole list (fp32)
def resolve(keys, h_d, w_d, rel, values):
    """values: the sources' (n_s, C) rows in the order of their ids.  -> (values (P,C), t (P,), src (P,) int32, empty (P,) bool,
    guard (P,) bool): ``empty`` and ``guard`` say WHY a pixel is a hole."""
    guard_f = F(1.0) + F(rel)
    P = h_d * w_d
    ends = np.cumsum([len(v) for v in values])
    Cn = values[0].shape[1]
    out = np.zeros((P, Cn), F)
    t_out = np.full(P, np.nan, F)
    src = np.full(P, -1, np.int32)
    empty = keys == EMPTY
    guard = np.zeros(P, bool)
    grid = keys.reshape(h_d, w_d)
    for j in range(P):
        if empty[j]:
            continue
        y, x = divmod(j, w_d)
        near = np.sort(grid[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1))[0]   # an empty key is the largest there is
        tp = np.array([int(keys[j]) >> 32], np.uint32).view(F)[0]
        m = np.array([int(near) >> 32], np.uint32).view(F)[0]
        with np.errstate(all="ignore"):
            bound = m * guard_f
        ident = int(keys[j]) & 0xFFFFFFFF
        s = int(np.searchsorted(ends, ident, side="right"))
        if tp > bound or s >= len(values):
            guard[j] = True
            continue
        row = ident - (int(ends[s - 1]) if s else 0)
        out[j], t_out[j], src[j] = values[s][row], tp, ident
    return out, t_out, src, empty, guard


def holes_of(src):
    return np.flatnonzero(np.asarray(src) < 0).astype(np.int32)


def reproject(sources, K_d, T_d, h_d, w_d, rel=REL, z_min=Z_MIN, id_bases=None):
    """The whole restatement -> dict(values, t, src, holes, n_holes, empty, guard, keys, candidates)."""
    keys, candidates = splat(sources, K_d, T_d, h_d, w_d, z_min, id_bases)
    values, t, src, empty, guard = resolve(keys, h_d, w_d, rel, [s[4] for s in sources])
    holes = holes_of(src)
    return dict(values=values, t=t, src=src, holes=holes, n_holes=len(holes), empty=empty, guard=guard, keys=keys, candidates=candidates)


def census(result):
    """What a result exercised -> dict(empty holes, guard holes, collisions won by depth, exact ties won by id, filled)."""
    depth = tie = 0
    for tg, ks in result["candidates"].items():
        if len(ks) < 2:
            continue
        depth += int((ks[1] >> 32) > (ks[0] >> 32))
        tie += int((ks[1] >> 32) == (ks[0] >> 32) and (ks[1] & 0xFFFFFFFF) > (ks[0] & 0xFFFFFFFF))
    return dict(empty=int(result["empty"].sum()), guard=int(result["guard"].sum()), depth=depth, tie=tie, filled=int((result["src"] >= 0).sum()))


# ---------------------------------------------------------------------------------------- the fp64 geometric check
PIXEL_SLACK = 1e-3   # fp32 slack of a projected coordinate, in pixels: about 40 roundings of 2^-24 relative on terms that reach
#                      f x / z ~ 30 px and on world coordinates of a few units divided by z >= 1 and multiplied by f <= 29:
#                      40 * 6e-8 * 30 * a condition of a few ~ 2e-4 px; 1e-3 leaves room and is 1/500 of the 0.5 px it is added to
T_REL = 1e-5         # the issue's bound on t'


def geometry_errors(result, source_views, K_d, T_d, w_d):
    """For every filled pixel j: the point its source row names (fp64 ray of the source pixel, times the fp32 t of that row),
    projected into the destination in fp64 -> (largest |u - iu|, |v - iv| over the filled pixels, largest relative error of t').
    source_views: [(K, T, w, t)] in id order.  No fp32 step and no code of the restatement."""
    Kd = np.asarray(K_d, np.float64).reshape(3, 3)
    Td = np.asarray(T_d, np.float64).reshape(4, 4)
    Wd = np.linalg.inv(Td)
    ends = np.cumsum([len(v[3]) for v in source_views])
    worst_px = worst_t = 0.0
    for j in np.flatnonzero(result["src"] >= 0):
        ident = int(result["src"][j])
        s = int(np.searchsorted(ends, ident, side="right"))
        K, T, w, t = source_views[s]
        row = ident - (int(ends[s - 1]) if s else 0)
        Tm = np.asarray(T, np.float64).reshape(4, 4)
        cam = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3)) @ np.array([row % w, row // w, 1.0])
        cam = cam / np.linalg.norm(cam)
        p = Tm[:3, 3] + float(t[row]) * (Tm[:3, :3] @ cam)
        c = Wd[:3, :3] @ p + Wd[:3, 3]
        pix = Kd @ c
        u, v = pix[0] / pix[2], pix[1] / pix[2]
        worst_px = max(worst_px, abs(u - (j % w_d)), abs(v - (j // w_d)))
        dist = float(np.linalg.norm(p - Td[:3, 3]))
        worst_t = max(worst_t, abs(float(result["t"][j]) - dist) / dist)
    return worst_px, worst_t


# ---------------------------------------------------------------------------------------- the case set of the GPU tests
def view(orbit=0.0, dist=4.0, h=H, w=W, focal=None):
    return dict(orbit=orbit, dist=dist, h=h, w=w, focal=focal)


# name -> (sources [(view, n rows or None = all)], destination view, rel).  At the source's own camera the guard still makes the
# far side of the strip's silhouette a hole (far / near = 6 / 4 there); same_camera therefore takes rel = 1, above every ratio of
# neighbouring depths in this frame, and must come back whole.
CASES = {
    "same_camera": ([(view(), None)], view(), 1.0),
    "orbit_3": ([(view(), None)], view(3.0), REL),
    "orbit_15": ([(view(), None)], view(15.0), REL),
    "dist_4_to_3": ([(view(), None)], view(0.0, 3.0), REL),
    "other_K_19x29": ([(view(), None)], view(3.0, 4.0, 19, 29, 31.0), REL),
    "two_sources": ([(view(), None), (view(6.0), None)], view(3.0), REL),
    "tie_twice": ([(view(), None), (view(), None)], view(3.0), REL),
}
for _n in (1, 63, 64, 65, 391):
    CASES[f"truncated_{_n}"] = ([(view(), _n)], view(3.0), REL)


def build_case(name):
    """-> (sources [(K, kinv, T, h, w, values, t)], (K_d, T_d, h_d, w_d), rel)."""
    srcs, dst, rel = CASES[name]
    out = []
    for v, n in srcs:
        K, T = camera(v["h"], v["w"], v["orbit"], v["dist"], v["focal"])
        t, values = analytic_frame(K, T, v["h"], v["w"], n)
        out.append((K, kinv_of(K), T, v["h"], v["w"], values, t))
    K_d, T_d = camera(dst["h"], dst["w"], dst["orbit"], dst["dist"], dst["focal"])
    return out, (K_d, T_d, dst["h"], dst["w"]), rel


def oracle_case(name):
    srcs, (K_d, T_d, h_d, w_d), rel = build_case(name)
    return reproject([(s[1], s[2], s[3], s[4], s[5], s[6]) for s in srcs], K_d, T_d, h_d, w_d, rel, Z_MIN)
