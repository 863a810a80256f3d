"""Shared by tests/test_deep_cpu.py and tests/test_gpu_deep.py: deep frames (include/stnerf.h / DESIGN.md sections 4.2 and 7)
restated from that text in numpy, fp32, one rounding per operation in the order written -- which samples are kept, how they are cut
into segments, the 8-word record, the CSR layout; and the compositing of depth-tested elements on the list, with the lane striding and
the in-place wave scan (csrc/wave_prims.h: wave_scan_add) the sums go through."""
import numpy as np

F = np.float32
U = 2.0 ** -24


def gamma(m):
    """The rounding bound of a sum of m terms in any order, each a rounded product: (m + 1) u / (1 - (m + 1) u)."""
    return (m + 1) * U / (1 - (m + 1) * U)


# ---------------------------------------------------------------------------------------- the list
def np_kept(wm, w_min):
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(wm, F) <= F(w_min))


def np_deep(t, wm, colour, have, w_min=0.0, merge_dz=0.0):
    """t, wm (n,l,S), colour (n,l,S,3) as the compositor uses it, have (n,l) bool (the layer has output on the ray) ->
    (counts (n,) int32, offsets (n+1,) int64, records (total,8) fp32 whose word 7 holds the uint32 meta).  The kept samples of the
    layers with output, in (ray, layer, source index) order, are one flat list; a segment is a run of it."""
    t, wm, colour = np.asarray(t, F), np.asarray(wm, F), np.asarray(colour, F)
    n, l, S = t.shape
    kept = np_kept(wm, w_min) & np.asarray(have, bool)[:, :, None]
    r, i, k = np.nonzero(kept)                                        # C order: ray, then layer, then source index
    if r.size == 0:
        return np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros((0, 8), F)
    first = np.ones(r.size, bool)                                     # the layer's first kept sample on the ray
    first[1:] = (r[1:] != r[:-1]) | (i[1:] != i[:-1])
    tk, wk = t[r, i, k], wm[r, i, k]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if merge_dz > 0:
            t0 = tk[np.maximum.accumulate(np.where(first, np.arange(r.size), 0))]
            bins = np.floor(((tk - t0).astype(F) / F(merge_dz)).astype(F)).astype(F)
            start = first.copy()
            start[1:] |= bins[1:] != bins[:-1]                        # (a NaN bin differs from every bin, itself included)
        else:
            start = np.ones(r.size, bool)
        heads = np.flatnonzero(start)
        count = np.diff(np.append(heads, r.size))
        x = np.stack([colour[r, i, k, 0], colour[r, i, k, 1], colour[r, i, k, 2], tk, np.ones(r.size, F)], 1)
        wx = (wk[:, None] * x).astype(F)
        acc = np.zeros((heads.size, 5), F)
        for j in range(int(count.max())):                             # acc = acc + w x, ascending source index
            on = count > j
            acc[on] = (acc[on] + wx[heads[on] + j]).astype(F)
    records = np.zeros((heads.size, 8), F)
    records[:, 0:3], records[:, 3], records[:, 4] = acc[:, 0:3], acc[:, 4], acc[:, 3]
    records[:, 5], records[:, 6] = tk[heads], tk[heads + count - 1]
    records.view(np.uint32)[:, 7] = (i[heads] | k[heads] << 8 | count << 16).astype(np.uint32)
    counts = np.bincount(r[heads], minlength=n).astype(np.int32)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum(counts.astype(np.int64))
    return counts, offsets, records


def meta_of(records):
    m = np.ascontiguousarray(records, F).view(np.uint32)[:, 7]
    return (m & 0xFF).astype(np.int64), ((m >> 8) & 0xFF).astype(np.int64), (m >> 16).astype(np.int64)


# ---------------------------------------------------------------------------------------- the wave scan
def np_wave_total(v):
    """v (..., 64) fp32 -> the value lane 63 holds after wave_scan_add: row_shr 1, 2, 4, 8 inside the rows of 16, then lane 15 of
    rows 0 / 2 added to rows 1 / 3, then lane 31 added to rows 2 and 3."""
    v = np.array(v, F)
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in (1, 2, 4, 8):
            sel = lane[(lane % 16) >= d]
            new = v.copy()
            new[..., sel] = (v[..., sel - d] + v[..., sel]).astype(F)
            v = new
        new = v.copy()
        new[..., 16:32] = (v[..., 15:16] + v[..., 16:32]).astype(F)
        new[..., 48:64] = (v[..., 47:48] + v[..., 48:64]).astype(F)
        v = new
        new = v.copy()
        new[..., 32:64] = (v[..., 31:32] + v[..., 32:64]).astype(F)
    return new[..., 63]


# ---------------------------------------------------------------------------------------- the elements
def np_rows(elements):
    """elements (E,5) -> (a' (E,), z' (E,), order): a' = clamp(a, 0, 1) with a NaN as 0; an absent row (a' == 0 or z not finite) has
    a' = 0 and z' = +inf; order = the rows' indices ascending by z', stable."""
    el = np.asarray(elements, F).reshape(-1, 5)
    with np.errstate(invalid="ignore"):
        ap = np.where(el[:, 3] > 0, el[:, 3], F(0)).astype(F)
        ap = np.where(ap < 1, ap, F(1)).astype(F)
    present = (ap > 0) & np.isfinite(el[:, 4])
    ap = np.where(present, ap, F(0)).astype(F)
    z = np.where(present, el[:, 4], F(np.inf)).astype(F)
    return ap, z, np.argsort(z, kind="stable")


def np_deep_composite(offsets, records, l, elements=None):
    """offsets (n+1,), records (total,8), elements (n,E,5) | None -> (mixed (n,5), scene (n,l,5), shares (n,E,5)), fp32."""
    offsets, records = np.asarray(offsets, np.int64), np.ascontiguousarray(records, F)
    n = offsets.shape[0] - 1
    E = 0 if elements is None else np.asarray(elements).shape[1]
    layer_all, _, _ = meta_of(records) if records.shape[0] else (np.zeros(0, np.int64),) * 3
    mixed, scene, shares = np.zeros((n, 5), F), np.zeros((n, l, 5), F), np.zeros((n, E, 5), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(n):
            lo, hi = int(offsets[r]), int(offsets[r + 1])
            rec, layer = records[lo:hi], layer_all[lo:hi]
            if E:
                ap, z, order = np_rows(np.asarray(elements, F)[r])
                a_s, z_s = ap[order], z[order]
            else:
                a_s, z_s, order = np.zeros(0, F), np.zeros(0, F), np.zeros(0, np.int64)
            P = np.ones(E + 1, F)
            for j in range(E):
                P[j + 1] = F(P[j] * F(F(1) - a_s[j]))
            zf = rec[:, 5]
            q = np.ones(hi - lo, F)
            behind = np.zeros((hi - lo, E), bool)
            for j in range(E):
                behind[:, j] = zf >= z_s[j]
                q = np.where(behind[:, j], P[j + 1], q).astype(F)
            x = rec[:, [0, 1, 2, 4, 3]]                                   # {r, g, b, zw, a}
            acc = np.zeros((l, 64, 5), F)
            af = np.zeros((64, E), F)
            for b0 in range(0, hi - lo, 64):
                d = np.arange(b0, min(b0 + 64, hi - lo))
                lanes = d - b0
                term = (q[d, None] * x[d]).astype(F)
                acc[layer[d], lanes] = (acc[layer[d], lanes] + term).astype(F)
                if E:
                    af[lanes] = (af[lanes] + np.where(behind[d], F(0), rec[d, 3:4])).astype(F)
            passes = np_wave_total(acc.transpose(0, 2, 1))                # (l,5)
            scene[r] = passes
            total = passes[0].copy()
            for i in range(1, l):
                total = (total + passes[i]).astype(F)
            if E:
                Af = np_wave_total(af.T)                                  # (E,)
                left = (F(1) - Af).astype(F)
                T = np.where(left > 0, left, F(0)).astype(F)
                s = ((a_s * T).astype(F) * P[:E]).astype(F)
                el = np.asarray(elements, F)[r][order]
                xs = np.stack([el[:, 0], el[:, 1], el[:, 2], z_s, np.ones(E, F)], 1)
                share = np.where((a_s > 0)[:, None], (s[:, None] * xs).astype(F), F(0)).astype(F)
                for j in range(E):
                    total = (total + share[j]).astype(F)
                shares[r, order] = share
            mixed[r] = total
    return mixed, scene, shares


def exact_deep_composite(offsets, records, l, elements=None):
    """The same quantities in fp64 from the fp32 records and rows, in any order -> (mixed, scene, shares, magnitude (n,5)):
    magnitude = sum over the ray's samples of |x|, the scale of the rounding bound of the passes."""
    offsets, rec64 = np.asarray(offsets, np.int64), np.ascontiguousarray(records, F).astype(np.float64)
    n = offsets.shape[0] - 1
    E = 0 if elements is None else np.asarray(elements).shape[1]
    layer_all = meta_of(records)[0] if records.shape[0] else np.zeros(0, np.int64)
    mixed, scene, shares, mag = np.zeros((n, 5)), np.zeros((n, l, 5)), np.zeros((n, E, 5)), np.zeros((n, 5))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(n):
            lo, hi = int(offsets[r]), int(offsets[r + 1])
            rec, layer = rec64[lo:hi], layer_all[lo:hi]
            x = rec[:, [0, 1, 2, 4, 3]]
            q = np.ones(hi - lo)
            if E:
                ap, z, order = np_rows(np.asarray(elements, F)[r])
                a_s, z_s = ap[order].astype(np.float64), z[order]
                zf = np.ascontiguousarray(records, F)[lo:hi, 5]
                behind = zf[:, None] >= z_s[None, :]
                q = np.where(behind, 1 - a_s[None, :], 1.0).prod(1)
            for i in range(l):
                scene[r, i] = (q[:, None] * x)[layer == i].sum(0)
            mag[r] = np.abs(x).sum(0)
            mixed[r] = scene[r].sum(0)
            if E:
                Af = np.where(behind, 0.0, rec[:, 3:4]).sum(0)
                T = np.where(1 - Af > 0, 1 - Af, 0.0)                  # (a NaN leaves nothing)
                P = np.concatenate([[1.0], np.cumprod(1 - a_s)])[:E]
                s = a_s * T * P
                el = np.asarray(elements, F)[r][order].astype(np.float64)
                xs = np.stack([el[:, 0], el[:, 1], el[:, 2], z_s.astype(np.float64), np.ones(E)], 1)
                share = np.where((a_s > 0)[:, None], s[:, None] * xs, 0.0)
                shares[r, order] = share
                mixed[r] += share.sum(0)
    return mixed, scene, shares, mag
