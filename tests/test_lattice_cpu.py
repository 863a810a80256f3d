"""Adaptive lattice frames, the host side (no GPU): ``LatticeSpec``'s validation, the driver's refusals, the library's argument
checks, and the properties of the numpy restatement (tests/lattice_common.py) the GPU tests are pinned to -- including that the
constructed fields fill AND queue pixels at every level, so that those tests cannot pass vacuously."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import lattice_common as L
from stnerf_amd import hip, lattice, parallel

F = np.float32
WITH_CELLS = [s for s in L.SHAPES if L.covered(*s)[2]]


# ---------------------------------------------------------------------------------------- the spec
def test_spec_defaults_and_validation():
    import stnerf_amd
    assert stnerf_amd.LatticeSpec is lattice.LatticeSpec
    s = lattice.LatticeSpec(2, 0.01)
    assert (s.levels, s.stride, s.tol_rgb, s.tol_depth, s.tol_alpha, s.force) == (2, 4, 0.01, math.inf, math.inf, "performers")
    assert s.strides() == [4, 2] and lattice.LatticeSpec(0, 0.0).strides() == [] and lattice.LatticeSpec(4, 1.0).strides() == [16, 8, 4, 2]
    with pytest.raises(TypeError):
        lattice.LatticeSpec(2)                                           # tol_rgb has no default
    for bad in (dict(levels=-1, tol_rgb=0.1), dict(levels=5, tol_rgb=0.1), dict(levels=1.5, tol_rgb=0.1), dict(levels=2, tol_rgb=-1e-9),
                dict(levels=2, tol_rgb=float("nan")), dict(levels=2, tol_rgb=0.1, tol_depth=-1.0), dict(levels=2, tol_rgb=0.1, tol_alpha=float("nan")),
                dict(levels=2, tol_rgb=0.1, force="everything"), dict(levels=2, tol_rgb=0.1, force=torch.zeros(4, 4)),
                dict(levels=2, tol_rgb=0.1, force=torch.zeros(16, dtype=torch.uint8)), dict(levels=2, tol_rgb=0.1, force=np.zeros((4, 4), np.uint8))):
        with pytest.raises(ValueError):
            lattice.LatticeSpec(**bad)
    assert lattice.LatticeSpec(1, 0.0, force=None).force is None
    mask = torch.ones(4, 4, dtype=torch.uint8)
    assert lattice.LatticeSpec(1, 0.0, force=mask).force is mask
    assert lattice.as_spec(dict(levels=3, tol_rgb=0.5)).levels == 3 and lattice.as_spec(s) is s
    with pytest.raises(TypeError):
        lattice.as_spec(3)
    # the tolerance vector: [rgb x 3, depth, alpha] over the mixed five and each layer's five; the package's is the restatement's
    t = lattice.LatticeSpec(2, 0.25, 0.5, 2.0).tolerances(2)
    assert t == [0.25, 0.25, 0.25, 0.5, 2.0] * 3 and len(t) == L.width(2) - L.E
    assert np.array_equal(np.asarray(t, F), L.tolerances(2, 0.25, 0.5, 2.0))
    assert all(math.isinf(x) for x in lattice.LatticeSpec(2, 0.25).tolerances(1)[3:5])
    for h, w, K in L.SHAPES + [(1080, 1920, 4), (24, 32, 2)]:
        assert lattice.covered(h, w, K) == L.covered(h, w, K)[:2]


# ---------------------------------------------------------------------------------------- the driver's refusals
def _fake_model(**over):
    m = types.SimpleNamespace(total_layers=3, layer_num=2, seed=5, fresh_draws_per_call=True, replay=None, ray_window=(0, 0, 0),
                              _bkgd_cache=None, _layer_cache=None, _occupancy=None, shard_views=False)
    for k, v in over.items():
        setattr(m, k, v)
    return m


K, T = torch.eye(3), torch.eye(4)
IDS = [1.0, 2.0, 3.0]


def test_the_driver_names_what_it_refuses(monkeypatch):
    """Every refusal is raised before anything touches the device (there is none here) and leaves the seed alone."""
    spec = lattice.LatticeSpec(2, 0.01)
    call = lambda model, spec=spec, **kw: parallel.render_view_lattice(model, K, T, 8, 8, IDS, spec, 0.0, 0.0, device="cpu", **kw)
    for over, what in ((dict(_bkgd_cache=object()), "sparse list"), (dict(_layer_cache=object()), "sparse list"),
                       (dict(replay={"jitter": None}), "replay")):
        m = _fake_model(**over)
        with pytest.raises(ValueError, match=what):
            call(m)
        assert m.seed == 5
    with pytest.raises(ValueError, match="out of scope"):
        call(_fake_model(), scene=True)
    with pytest.raises(ValueError, match="out of scope"):
        call(_fake_model(), occluder=torch.zeros(64, 5))
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        call(_fake_model(), accumulate=dict(max_spp=2))
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        call(_fake_model(), reproject=(object(), []))
    with pytest.raises(ValueError, match="aperture"):
        call(_fake_model(), lens=dict(aperture=0.1, focus=3.0))
    with pytest.raises(ValueError, match=r"\(8,8\)"):
        call(_fake_model(), lattice.LatticeSpec(2, 0.01, force=torch.zeros(4, 4, dtype=torch.uint8)))
    with pytest.raises(TypeError):
        call(_fake_model(), 3)
    monkeypatch.setattr(parallel, "active_group", lambda model=None: (0, 2, None))
    with pytest.raises(RuntimeError, match="one rank"):
        call(_fake_model(shard_views=True))


def test_render_pose_and_the_renderer_refuse_the_same_combinations():
    from stnerf_amd.render import LayeredNeuralRenderer
    from stnerf_amd.render.render_pose import render_pose
    m, pairs, spec = _fake_model(), list(enumerate(IDS)), lattice.LatticeSpec(2, 0.01)
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(m, T, K, 8, 8, pairs, 20.0, lattice=spec, scene_passes=True, device="cpu")
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(m, T, K, 8, 8, pairs, 20.0, lattice=dict(levels=2, tol_rgb=0.01), device="cpu", occluder=(torch.zeros(8, 8, 4), torch.zeros(8, 8)))
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        render_pose(m, T, K, 8, 8, pairs, 20.0, lattice=spec, accumulate=dict(max_spp=2), device="cpu")
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        render_pose(m, T, K, 8, 8, pairs, 20.0, lattice=spec, reproject=(dict(key_every=2), []), device="cpu")
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[8, 8]), OUTPUT_DIR="")
    make = lambda **kw: LayeredNeuralRenderer(cfg, model=_fake_model(), gt_poses=T[None], gt_Ks=[K], lattice=spec, **kw)
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        make(accumulate=dict(max_spp=2))
    with pytest.raises(ValueError, match="out of scope"):
        make(scene_passes=True)
    with pytest.raises(ValueError, match="out of scope"):
        make(occluder=lambda idx, pose, K: None)
    r = make()
    assert r.lattice is spec and r.lattice_stats == []


# ---------------------------------------------------------------------------------------- the library's host checks
def test_entries_check_their_arguments_before_any_launch():
    lib = hip.lib()
    fake, null = C.c_void_p(1 << 20), C.c_void_p(0)           # (never dereferenced)
    begin = lambda h=9, w=9, levels=2, status=fake: lib.stnerf_lattice_begin(h, w, levels, null, status, None)
    for bad in (begin(h=0), begin(w=0), begin(h=1 << 16, w=1 << 16), begin(levels=-1), begin(levels=5), begin(status=null)):
        assert bad == hip.EINVAL
    assert begin(levels=5) == hip.EINVAL and "outside 0..4" in hip.last_error()
    cls = lambda h=9, w=9, Cw=11, Ew=1, levels=2, s=4, tol=fake, flat=fake, nflat=81, values=fake, status=fake: lib.stnerf_lattice_classify(
        values, status, h, w, Cw, Ew, levels, s, tol, flat, nflat, None)
    for bad in (cls(h=0), cls(h=1 << 16, w=1 << 16), cls(levels=5), cls(levels=-1), cls(s=1), cls(s=3), cls(s=8), cls(s=0), cls(levels=0, s=2),
                cls(Cw=0), cls(Cw=4097), cls(Ew=-1), cls(Ew=12), cls(tol=null), cls(flat=null), cls(values=null), cls(status=null),
                cls(nflat=3), cls(s=2, nflat=15)):
        assert bad == hip.EINVAL
    assert cls(s=3) == hip.EINVAL and "power of two" in hip.last_error()
    assert cls(nflat=3) == hip.EINVAL and "flat bytes" in hip.last_error()
    assert cls(h=5, w=3, levels=3, s=8, nflat=0) == hip.OK               # no cell: nothing to do, no launch
    ws = lib.stnerf_lattice_select_workspace_bytes
    assert [ws(P) for P in (1, 256, 64 * 256, 64 * 256 + 1, 1920 * 1080)] == [256, 256, 256, 512, 32512]
    assert ws(0) == hip.EINVAL and ws(1 << 31) == hip.EINVAL
    sel = lambda P=1000, nbytes=256, out=fake, work=fake, status=fake, n_out=fake: lib.stnerf_lattice_select(status, P, out, n_out, work, nbytes, None)
    for bad in (sel(P=0), sel(P=1 << 31), sel(out=null), sel(work=null), sel(status=null), sel(n_out=null), sel(P=70001, nbytes=1024)):
        assert bad == hip.EINVAL
    assert sel(P=70001, nbytes=1024) == hip.EINVAL and "workspace too small" in hip.last_error()
    sca = lambda n=10, Cw=11, stride=11, P=81, rows=fake, pixels=fake, values=fake, status=fake: lib.stnerf_lattice_scatter(
        rows, n, Cw, stride, pixels, P, values, status, None)
    assert sca(n=0) == hip.OK                                             # nothing to do: no launch
    for bad in (sca(n=82), sca(n=-1), sca(stride=10), sca(Cw=0), sca(Cw=4097), sca(P=0), sca(P=1 << 31), sca(rows=null), sca(pixels=null),
                sca(values=null), sca(status=null)):
        assert bad == hip.EINVAL
    assert sca(stride=10) == hip.EINVAL and "stride" in hip.last_error()


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from stnerf_amd import ops
    state = ops.lattice_state(4, 6, 11, device="cpu")
    assert state.values.shape == (24, 11) and state.status.dtype == torch.uint8 and state.n_pixels == 24 and not state.status.any()
    with pytest.raises(ValueError):
        ops.lattice_state(0, 6, 11, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.lattice_begin(state, 2)
    with pytest.raises(ValueError, match="force must be"):
        ops.lattice_begin(state, 2, torch.zeros(6, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="one bound per tested column"):
        ops.lattice_classify(state, 2, 4, torch.zeros(11))
    with pytest.raises(ValueError, match="floats wide"):
        ops.lattice_scatter(torch.zeros(3, 10), state, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="pixels must be"):
        ops.lattice_scatter(torch.zeros(3, 11), state, torch.zeros(4, dtype=torch.int32))


# ---------------------------------------------------------------------------------------- the restatement's own properties
def levels_of(h, w, K, l):
    """The loop on the constructed field, level by level -> [(s, values before, status before, values after, status after)]."""
    truth, tol, force = L.field(h, w, K, l)
    values, status = np.zeros_like(truth), L.begin(h, w, K, force)
    out = []
    for s in L.strides(K):
        pix = L.select(status)
        L.scatter(values, status, truth[pix], pix)
        before = (values.copy(), status.copy())
        counts = L.classify(values, status, h, w, K, s, tol)
        out.append((s, *before, values.copy(), status.copy(), counts))
    pix = L.select(status)
    L.scatter(values, status, truth[pix], pix)
    return truth, tol, force, values, status, out


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("h,w,K", L.SHAPES)
def test_begin_and_the_end_of_the_loop(h, w, K, l):
    truth, tol, force, values, status, levels = levels_of(h, w, K, l)
    S = 1 << K
    first = L.begin(h, w, K, force)
    Wc, Hc, cells = L.covered(h, w, K)
    for y in range(h):
        for x in range(w):
            margin = not cells or x > Wc or y > Hc
            assert (first[y * w + x] == L.QUEUED) == bool(margin or force[y, x] or (x % S == 0 and y % S == 0)), (x, y)
    if not cells or K == 0:
        assert (first == L.QUEUED).all()
    # after the last level no pixel is unknown or queued; a rendered pixel holds the truth's bits, the margin is rendered
    assert set(np.unique(status)) <= {L.RENDERED, L.FILLED}
    r = status == L.RENDERED
    assert np.array_equal(values[r].view(np.uint32), truth[r].view(np.uint32))
    assert all(status[y * w + x] == L.RENDERED for y in range(h) for x in range(w) if L.is_margin(x, y, h, w, K) or force[y, x])
    # the run() loop is this loop
    v2, s2, rays, counts = L.run(h, w, K, truth.shape[1], tol, lambda pix: truth[pix], force)
    assert np.array_equal(v2.view(np.uint32), values.view(np.uint32)) and np.array_equal(s2, status)
    assert len(rays) == K + 1 and sum(rays) == int(r.sum()) and counts == [lv[-1] for lv in levels]


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("h,w,K", WITH_CELLS)
def test_the_constructed_fields_fill_and_queue_at_every_level(h, w, K, l):
    """What keeps the GPU tests from passing vacuously: every level of every field with cells fills some pixels and queues others,
    the NaN corner, the -0 corner and the exact column's change each sit on a lattice point of a cell, and at some level a cell is
    refused by its exact column alone."""
    truth, tol, force, values, status, levels = levels_of(h, w, K, l)
    assert [lv[0] for lv in levels] == L.strides(K)
    for s, vb, sb, va, sa, (filled, queued) in levels:
        print(f"{h}x{w} K={K} l={l} stride {s}: filled {filled}, queued {queued}")
        assert filled > 0 and queued > 0, (s, filled, queued)
    Wc, Hc, _ = L.covered(h, w, K)
    C = truth.shape[1]
    assert np.isnan(truth[Hc * w, 0]) and np.signbit(truth[0, 3]) and truth[0, 3] == 0 and not np.signbit(truth[1:, 3]).any()
    assert (force != 0).any() and not (force != 0).all()
    by_exact_alone = 0
    for s, vb, sb, va, sa, _ in levels:
        for cy in range(0, Hc, s):
            for cx in range(0, Wc, s):
                q = L.corners(w, cx, cy, s)
                if (sb[q] == L.UNKNOWN).any():
                    continue
                loose = vb.copy()
                loose[:, C - 1] = 1.0
                by_exact_alone += (not L.cell_flat(vb, w, cx, cy, s, tol)) and L.cell_flat(loose, w, cx, cy, s, tol)
    assert by_exact_alone > 0


@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("h,w,K", WITH_CELLS)
def test_a_filled_value_lies_between_its_cells_corners(h, w, K, l):
    """Per tested column, up to 1 ulp of the larger corner; an exact column is v00's; a pixel is filled only if EVERY cell around
    it is flat, and from the first of them."""
    truth, tol, force, values, status, levels = levels_of(h, w, K, l)
    C = truth.shape[1]
    n_edge = n_edge_refused = 0
    for s, vb, sb, va, sa, _ in levels:
        for q in np.flatnonzero(sb == L.UNKNOWN):
            x, y = int(q % w), int(q // w)
            around = L.cells_around(x, y, s, h, w, K)
            if not around:
                continue
            flats = [L.cell_flat(vb, w, cx, cy, s, tol) for cx, cy in around]
            assert len(around) in (1, 2) and around == sorted(around, key=lambda c: (c[1], c[0]))
            n_edge += len(around) == 2
            if not all(flats):
                n_edge_refused += len(around) == 2 and any(flats)
                assert sa[q] == (L.QUEUED if x % (s // 2) == 0 and y % (s // 2) == 0 else L.UNKNOWN)
                assert np.array_equal(va[q].view(np.uint32), vb[q].view(np.uint32))
                continue
            assert sa[q] == L.FILLED
            cx, cy = around[0]
            want = L.interpolate(vb, w, x, y, cx, cy, s)
            assert np.array_equal(va[q].view(np.uint32), want.view(np.uint32))
            four = vb[L.corners(w, cx, cy, s)]
            lo, hi = four[:, :C - 1].min(0), four[:, :C - 1].max(0)
            ulp = np.spacing(np.abs(four[:, :C - 1]).max(0))
            assert (va[q, :C - 1] >= lo - ulp).all() and (va[q, :C - 1] <= hi + ulp).all(), (x, y, s)
            assert va[q, C - 1] == four[0, C - 1]
    assert n_edge > 0 and n_edge_refused > 0        # edges between two cells occur, also between a flat and a refused cell


def test_flat_is_finite_spread_within_the_bound_and_equal_exact_columns():
    w, tol = 3, np.asarray([0.5, np.inf], F)
    base = np.zeros((9, 3), F)
    base[:, 2] = 7.0
    flat = lambda v: L.cell_flat(v, w, 0, 0, 2, tol)
    assert flat(base)
    for q, c, value, want in ((0, 0, 0.5, True), (8, 0, np.nextafter(F(0.5), F(1)), False), (2, 0, np.nan, False), (6, 0, np.inf, False),
                              (0, 1, 1e30, True), (0, 1, -np.inf, False), (0, 1, np.nan, False), (8, 2, 7.5, False), (8, 2, np.nan, False),
                              (4, 0, np.nan, True), (4, 2, 9.0, True), (0, 0, -0.0, True)):
        v = base.copy()
        v[q, c] = value
        assert flat(v) == want, (q, c, value)
    zero = base.copy()
    zero[:, 2] = 0.0
    zero[0, 2] = -0.0
    assert flat(zero)                                                    # -0 == +0
    nan_tol = np.asarray([np.nan, np.inf], F)
    assert not L.cell_flat(base, w, 0, 0, 2, nan_tol)                    # a NaN bound is never met


def test_a_point_on_a_shared_edge_takes_the_first_cells_value():
    """Two flat cells side by side, stride 2, on a 3 x 5 view: the edge pixel (2, 1) is filled from the cell at cx = 0, where
    fx = 1: v = gy (0 v00 + 1 v10) + fy (0 v01 + 1 v11) -- with a -0 at v10 and v11 the products' zeros decide the sign, and the
    exact column is that cell's v00."""
    h, w, K = 3, 5, 1
    values, status = np.zeros((15, 2), F), L.begin(h, w, K)
    lattice_points = [q for q in range(15) if (q % w) % 2 == 0 and (q // w) % 2 == 0]
    assert L.select(status).tolist() == lattice_points
    rows = np.zeros((len(lattice_points), 2), F)
    rows[:, 1] = 4.0
    rows[[1, 2, 4, 5], 0] = -0.0                                         # the points (2, 0), (2, 2) -- the shared edge's ends -- and (4, 0), (4, 2)
    L.scatter(values, status, rows, lattice_points)
    filled, queued = L.classify(values, status, h, w, K, 2, np.asarray([0.0], F))
    assert (filled, queued) == (9, 0) and status[1 * w + 2] == L.FILLED
    assert L.cells_around(2, 1, 2, h, w, K) == [(0, 0), (2, 0)]
    first, second = L.interpolate(values, w, 2, 1, 0, 0, 2), L.interpolate(values, w, 2, 1, 2, 0, 2)
    got = values[1 * w + 2]
    assert np.array_equal(got.view(np.uint32), first.view(np.uint32)) and got[1] == 4.0
    assert not np.signbit(first[0]) and np.signbit(second[0])            # (+0) + (-0) = +0 from the first cell, -0 from the second
