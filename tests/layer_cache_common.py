"""Shared by the layer cache's tests: the listed copy restated in numpy from include/stnerf.h (section "the layer cache"), the
argument errors of stnerf_copy_layer_raw_listed (no launch is made: they run without a GPU too), and the lists the tests use."""
import ctypes as C

import numpy as np

from stnerf_amd import hip


def listed_copy_reference(raw, layer, dense, rays, count, to_dense, ray_list=None, ray_count=None, mismatch=0):
    """-> (raw, dense, rays, count, mismatch) after stnerf_copy_layer_raw_listed, on copies of the inputs.
    raw (n,l,ns,4), dense (capacity,ns,4), rays (capacity,) int32, count: an int; ray_list (>= ray_count entries) / ray_count: the
    frame's list (capture), or just the frame's count (restore, for the mismatch counter)."""
    raw, dense, rays = raw.copy(), dense.copy(), rays.copy()
    capacity = dense.shape[0]
    if to_dense:
        c = int(ray_count)
        if 0 <= c <= capacity:
            count = c
            rays[:c] = ray_list[:c]
            dense[:c] = raw[ray_list[:c], layer]
        else:
            count = -1
    else:
        c = int(count)
        if 0 <= c <= capacity:
            raw[rays[:c], layer] = dense[:c]
        if ray_count is not None and int(ray_count) != c:
            mismatch += 1
    return raw, dense, rays, count, mismatch


def listed_copy_loop(raw, layer, dense, rays, count, to_dense, ray_list=None, ray_count=None, mismatch=0):
    """The same rule as a plain loop over slots and samples (what the numpy restatement is checked against)."""
    raw, dense, rays = raw.copy(), dense.copy(), rays.copy()
    capacity, ns = dense.shape[0], dense.shape[1]
    if to_dense:
        c = int(ray_count)
        if c > capacity or c < 0:
            return raw, dense, rays, -1, mismatch
        for j in range(c):
            rays[j] = ray_list[j]
            for k in range(ns):
                for q in range(4):
                    dense[j, k, q] = raw[ray_list[j], layer, k, q]
        return raw, dense, rays, c, mismatch
    c = int(count)
    if ray_count is not None and int(ray_count) != c:
        mismatch += 1
    if c > capacity:
        c = 0
    for j in range(max(c, 0)):
        for k in range(ns):
            for q in range(4):
                raw[rays[j], layer, k, q] = dense[j, k, q]
    return raw, dense, rays, count, mismatch


def ray_lists(n, rs):
    """The lists of the tests, as (name, int32 array of distinct rays): empty, every ray (shuffled), a shuffled subset."""
    every = rs.permutation(n).astype(np.int32)
    subset = rs.permutation(n)[:max(1, n // 3)].astype(np.int32) if n > 1 else every.copy()
    return [("empty", np.zeros(0, np.int32)), ("every ray", every), ("subset", subset)]


def check_listed_copy_argument_errors():
    """Every STNERF_EINVAL of stnerf_copy_layer_raw_listed, with made-up pointers: each is refused before any launch."""
    lib = hip.lib()
    fake = 1 << 20                                     # (16-byte aligned, never dereferenced)
    null = C.c_void_p(0)

    def call(raw=fake, n=8, l=3, layer=1, ns=4, ray_list=fake, ray_count=fake, dense=fake, rays=fake, count=fake, capacity=8, to_dense=1,
             mismatch=null):
        return lib.stnerf_copy_layer_raw_listed(raw, n, l, layer, ns, ray_list, ray_count, dense, rays, count, capacity, to_dense, mismatch, None)

    bad = [
        (dict(layer=0), "not a performer"), (dict(layer=3), "not a performer"), (dict(layer=-1), "not a performer"),
        (dict(ns=0), "bad shape"), (dict(capacity=-1), "negative capacity"),
        (dict(raw=null), "null pointer"), (dict(dense=null), "null pointer"), (dict(rays=null), "null pointer"),
        (dict(count=null), "null pointer"), (dict(ray_list=null), "ray list"), (dict(ray_count=null), "ray list"),
        (dict(raw=fake + 4), "16-byte aligned"), (dict(dense=fake + 8), "16-byte aligned"),
        (dict(to_dense=0, mismatch=fake + 4), "8-byte aligned"), (dict(l=1, layer=1), "bad shape"), (dict(n=-1), "bad shape"),
    ]
    for kw, message in bad:
        for to_dense in ((kw["to_dense"],) if "to_dense" in kw else (1, 0)):
            if not to_dense and ("ray_list" in kw or "ray_count" in kw):
                continue                                # (a restore needs neither)
            assert call(**{**kw, "to_dense": to_dense}) == hip.EINVAL, (kw, to_dense)
            assert message in hip.last_error(), (kw, hip.last_error())
    return len(bad)
