"""The numpy restatement of adaptive lattice frames (include/stnerf.h: stnerf_lattice_begin,
stnerf_lattice_classify, stnerf_lattice_select, stnerf_lattice_scatter): the first queue, the flat test of a cell, the fill and
the status of a level, the list of queued pixels, the scatter and the whole level loop, in fp32 throughout, ONE operation per
line, so that numpy rounds after every operation as the kernels (built without contraction) do.  Restated from the definitions,
not from the package: nothing here imports it.  Also the constructed fields the CPU and the GPU tests share."""
import numpy as np

F = np.float32
UNKNOWN, RENDERED, FILLED, QUEUED = 0, 1, 2, 3
E = 1                                           # the exact columns: the hit-mask bits, the last one


def width(l):
    """C of ``pack_outputs(raw, "fine")``: mixed 5, l layers of 5, the mask bits."""
    return 6 + 5 * l


def tolerances(l, tol_rgb, tol_depth=np.inf, tol_alpha=np.inf):
    five = [tol_rgb, tol_rgb, tol_rgb, tol_depth, tol_alpha]
    return np.asarray(five * (1 + l), F)


def covered(h, w, K):
    """(Wc, Hc, any cell at all)."""
    S = 1 << K
    Wc = (w - 1) // S * S
    Hc = (h - 1) // S * S
    return Wc, Hc, Wc > 0 and Hc > 0


def is_margin(x, y, h, w, K):
    Wc, Hc, cells = covered(h, w, K)
    return (not cells) or x > Wc or y > Hc


# ---------------------------------------------------------------------------------------- begin
def begin(h, w, K, force=None):
    """status (h w,) uint8: 3 on the margin, where force is nonzero and on the top lattice; 0 elsewhere."""
    S = 1 << K
    status = np.zeros(h * w, np.uint8)
    for y in range(h):
        for x in range(w):
            q = y * w + x
            forced = force is not None and np.asarray(force).reshape(-1)[q] != 0
            if is_margin(x, y, h, w, K) or forced or (x % S == 0 and y % S == 0):
                status[q] = QUEUED
    return status


# ---------------------------------------------------------------------------------------- flat cells
def corners(w, cx, cy, s):
    """q of v00, v10, v01, v11."""
    return [cy * w + cx, cy * w + cx + s, (cy + s) * w + cx, (cy + s) * w + cx + s]


def cell_flat(values, w, cx, cy, s, tol, exact=E):
    v = values[corners(w, cx, cy, s)]                                   # (4, C)
    T = values.shape[1] - exact
    for c in range(T):
        four = v[:, c]
        if not np.isfinite(four).all():
            return False
        hi = four.max()
        lo = four.min()
        spread = F(hi - lo)                                             # one fp32 subtraction
        if not spread <= tol[c]:
            return False
    for c in range(T, values.shape[1]):
        four = v[:, c]
        if not (four[0] == four[1] and four[0] == four[2] and four[0] == four[3]):
            return False
    return True


def cells_around(x, y, s, h, w, K):
    """The cells of stride s whose closure contains (x, y), inside the covered region: lowest cy first, then lowest cx."""
    Wc, Hc, cells = covered(h, w, K)
    if not cells or x > Wc or y > Hc:
        return []
    xs = [x - s, x] if x % s == 0 else [x // s * s]
    ys = [y - s, y] if y % s == 0 else [y // s * s]
    return [(cx, cy) for cy in ys for cx in xs if cx >= 0 and cy >= 0 and cx + s <= Wc and cy + s <= Hc]


# ---------------------------------------------------------------------------------------- classify / fill
def interpolate(values, w, x, y, cx, cy, s, exact=E):
    """The filled row of (x, y) from the cell (cx, cy, s): every product and sum one fp32 operation."""
    v00, v10, v01, v11 = (values[q] for q in corners(w, cx, cy, s))
    T = values.shape[1] - exact
    fx = F(x - cx) / F(s)
    gx = F(1) - fx
    fy = F(y - cy) / F(s)
    gy = F(1) - fy
    with np.errstate(all="ignore"):
        t0 = gx * v00[:T]
        t1 = fx * v10[:T]
        top = t0 + t1
        b0 = gx * v01[:T]
        b1 = fx * v11[:T]
        bot = b0 + b1
        r0 = gy * top
        r1 = fy * bot
        row = r0 + r1
    assert row.dtype == F
    return np.concatenate([row, v00[T:]])


def classify(values, status, h, w, K, s, tol, exact=E):
    """One level, in place -> (pixels filled, pixels queued).  Reads the state as it was on entry."""
    assert 2 <= s <= (1 << K) and s & (s - 1) == 0
    before, was = values.copy(), status.copy()
    Wc, Hc, cells = covered(h, w, K)
    filled = queued = 0
    if not cells:
        return 0, 0
    flat = {}
    for cy in range(0, Hc, s):
        for cx in range(0, Wc, s):
            flat[(cx, cy)] = cell_flat(before, w, cx, cy, s, tol, exact)
    for y in range(Hc + 1):
        for x in range(Wc + 1):
            q = y * w + x
            if was[q] != UNKNOWN:
                continue
            around = cells_around(x, y, s, h, w, K)
            if around and all(flat[c] for c in around):
                cx, cy = around[0]
                values[q] = interpolate(before, w, x, y, cx, cy, s, exact)
                status[q] = FILLED
                filled += 1
            elif x % (s // 2) == 0 and y % (s // 2) == 0:
                status[q] = QUEUED
                queued += 1
    return filled, queued


# ---------------------------------------------------------------------------------------- select / scatter / the loop
def select(status):
    return np.flatnonzero(status == QUEUED).astype(np.int32)


def scatter(values, status, rows, pixels):
    P = status.shape[0]
    for i, q in enumerate(np.asarray(pixels, np.int64)):
        if 0 <= q < P:
            values[q] = rows[i]
            status[q] = RENDERED


def strides(K):
    return [1 << k for k in range(K, 0, -1)]


def run(h, w, K, C, tol, render, force=None, exact=E):
    """The whole loop.  render(pixels int32 ascending) -> rows (n, C) fp32; an empty list is not rendered.
    -> values, status, rays_per_level, [(filled, queued) per classified level]."""
    values, status = np.zeros((h * w, C), F), begin(h, w, K, force)
    rays, counts = [], []

    def render_queued():
        pix = select(status)
        rays.append(len(pix))
        if len(pix):
            scatter(values, status, np.asarray(render(pix), F), pix)

    for s in strides(K):
        render_queued()
        counts.append(classify(values, status, h, w, K, s, tol, exact))
    render_queued()
    return values, status, rays, counts


def top_cell_spread(values, h, w, K, cols):
    """max - min over the four corners, the largest over ``cols``, of every top-level cell of a full frame (fp32)."""
    S = 1 << K
    Wc, Hc, cells = covered(h, w, K)
    out = []
    if cells:
        for cy in range(0, Hc, S):
            for cx in range(0, Wc, S):
                v = values[corners(w, cx, cy, S)][:, cols]
                out.append(F(v.max(0) - v.min(0)).max())
    return np.asarray(out, F)


# ---------------------------------------------------------------------------------------- the constructed fields
SHAPES = [(9, 9, 2), (11, 13, 2), (17, 17, 3), (5, 3, 3), (1, 1, 0)]     # (h, w, K)
TOL_RGB, TOL_DEPTH = 0.01, 0.5


def field(h, w, K, l, seed=0):
    """A full frame to sample -> (truth (h w, C) fp32, tol (C - 1,) fp32, force (h, w) uint8).

    Colour and depth columns: a ramp a x + b y whose spread over a top cell, (a + b) S, is at most half the column's bound; plus
    a step of ten bounds at x >= xe, an odd x inside the last column of top cells (aligned to no lattice).  Alpha columns: noise
    (their bound is +inf: only finiteness is tested).  The mixed depth column is all +0 with a -0 at the lattice point (0, 0);
    colour column 0 is NaN at the lattice point (0, Hc); the exact column is 1, and 3 on the rows y >= Hc - 1 at 1 <= x <= S --
    it changes across cells whose tested columns are flat.  force: a random 10 % of the pixels."""
    rng = np.random.RandomState(1000 * h + 10 * w + K + 100 * l + seed)
    S = 1 << K
    C = width(l)
    tol = tolerances(l, TOL_RGB, TOL_DEPTH)
    Wc, Hc, cells = covered(h, w, K)
    xe = Wc - S + S // 2 + 1
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.reshape(-1), y.reshape(-1)
    truth = np.zeros((h * w, C), F)
    for c in range(C - E):
        kind = c % 5
        if kind == 4:
            truth[:, c] = rng.rand(h * w).astype(F)
            continue
        bound = TOL_RGB if kind < 3 else TOL_DEPTH
        a, b = (F(bound / (4.0 * S) * u) for u in rng.uniform(0.5, 1.0, 2))
        ax = a * x.astype(F)
        by = b * y.astype(F)
        ramp = ax + by
        ramp = ramp + F(rng.uniform(0.1, 0.9))
        step = np.where(x >= xe, F(10.0 * bound), F(0.0)).astype(F)
        truth[:, c] = ramp + step
    truth[:, 3] = F(0.0)
    truth[0, 3] = F(-0.0)
    truth[:, C - 1] = F(1.0)
    if cells:
        truth[Hc * w + 0, 0] = np.nan
        truth[(y >= Hc - 1) & (x >= 1) & (x <= S), C - 1] = F(3.0)
    force = (rng.rand(h, w) < 0.10).astype(np.uint8)
    return truth, tol, force
