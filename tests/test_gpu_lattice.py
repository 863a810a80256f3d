"""Adaptive lattice frames on the MI355X (csrc/lattice.hip): the first queue, the classify / fill of a level,
the ordered compaction of the queued pixels and the scatter against the numpy restatement of tests/lattice_common.py, bit for
bit, on the constructed fields tests/test_lattice_cpu.py shows to fill and queue at every level; then the driver
(``parallel.render_view_lattice``), ``render_pose(lattice=)`` and the renderer's ``lattice=`` on the small model of
tests/test_gpu_accumulate.py at 24 x 32 (768 rays; covered 29 x 21 at K = 2, a margin of three columns and three rows)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import lattice_common as L
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import bits, detach_models, same_bits
from stnerf_amd import hip, ops, parallel, synthetic as syn
from stnerf_amd.lattice import LatticeSpec

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x7FC0BEEF             # a NaN pattern no kernel writes
POISON_BYTE = 0xEE              # a status no kernel writes


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def assert_state(state, values, status, what):
    torch.cuda.synchronize()
    assert torch.equal(state.status, dev(status, np.uint8)), what
    assert torch.equal(bits(state.values), bits(dev(values, F))), what


# ---------------------------------------------------------------------------------------- op level: the whole loop, step by step
@pytest.mark.parametrize("l", [1, 3])
@pytest.mark.parametrize("h,w,K", L.SHAPES)
def test_every_step_of_the_loop_equals_the_restatement_bit_for_bit(h, w, K, l):
    truth, tol, force = L.field(h, w, K, l)
    C_ = truth.shape[1]
    truth_d, tol_d = dev(truth, F), dev(tol, F)
    state = ops.lattice_state(h, w, C_)
    values = np.zeros_like(truth)
    ops.lattice_begin(state, K, dev(force, np.uint8))
    status = L.begin(h, w, K, force)
    assert_state(state, values, status, "begin")

    def render_queued(what):
        pix, n = ops.lattice_select(state)
        want = L.select(status)
        assert n == len(want) and pix.dtype == torch.int32 and np.array_equal(pix.cpu().numpy(), want), what
        ops.lattice_scatter(truth_d[pix.long()], state, pix)
        L.scatter(values, status, truth[want], want)
        assert_state(state, values, status, what)
        return n

    rays = []
    for s in L.strides(K):
        rays.append(render_queued(f"list before stride {s}"))
        ops.lattice_classify(state, K, s, tol_d)
        filled, queued = L.classify(values, status, h, w, K, s, tol)
        assert_state(state, values, status, f"classify at stride {s}")
        print(f"{h}x{w} K={K} l={l} stride {s}: filled {filled}, queued {queued}")
    rays.append(render_queued("last list"))
    assert set(np.unique(status)) <= {L.RENDERED, L.FILLED} and rays[0] > 0
    if h * w > 256:
        assert rays[0] + rays[-1] < h * w and int(np.flatnonzero(status == L.RENDERED).max()) > 256      # lists cross a workgroup


def test_begin_without_a_force_mask_and_with_a_flat_one():
    h, w, K = 11, 13, 2
    state = ops.lattice_state(h, w, 11)
    ops.lattice_begin(state, K)
    torch.cuda.synchronize()
    assert torch.equal(state.status, dev(L.begin(h, w, K), np.uint8))
    force = (np.arange(h * w) % 7 == 3).astype(np.uint8)
    ops.lattice_begin(state, K, dev(force))                              # (h w,) is taken as (h, w)
    torch.cuda.synchronize()
    assert torch.equal(state.status, dev(L.begin(h, w, K, force), np.uint8))


# ---------------------------------------------------------------------------------------- scatter
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("Cw", [11, 21])
def test_scatter_writes_the_listed_pixels_and_nothing_else(Cw, pad):
    """P = 300 pixels inside guard rows on both sides of both arrays; 90 rows (row stride Cw + pad) at a shuffled list with four
    entries outside [0, P): those rows are dropped, the others land where the list says with status 1, every other byte stays."""
    P, G, n = 300, 5, 90
    rng = np.random.RandomState(Cw + pad)
    big_v = torch.full((P + 2 * G, Cw), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    big_s = torch.full((P + 2 * G,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    state = ops.lattice_state(1, P, Cw)
    state.values, state.status = big_v[G:G + P], big_s[G:G + P]
    pix = rng.choice(P, n, replace=False).astype(np.int32)
    pix[[3, 40, 41, 89]] = [-1, P, P + 2, 1 << 30]
    buf = rng.randn(n, Cw + pad).astype(F)
    rows = dev(buf)[:, :Cw]
    assert rows.stride(0) == Cw + pad
    ops.lattice_scatter(rows, state, dev(pix))
    torch.cuda.synchronize()
    want_v = np.full((P + 2 * G, Cw), POISON, np.int32)
    want_s = np.full(P + 2 * G, POISON_BYTE, np.uint8)
    inside = (pix >= 0) & (pix < P)
    assert inside.sum() == n - 4
    want_v[G + pix[inside]] = buf[inside, :Cw].view(np.int32)
    want_s[G + pix[inside]] = L.RENDERED
    assert torch.equal(bits(big_v), dev(want_v)) and torch.equal(big_s, dev(want_s))
    # an empty list: nothing at all
    ops.lattice_scatter(rows[:0], state, dev(pix[:0]))
    torch.cuda.synchronize()
    assert torch.equal(bits(big_v), dev(want_v)) and torch.equal(big_s, dev(want_s))


# ---------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("pattern", ["empty", "full", "random"])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 70001])
def test_select_equals_flatnonzero_of_status_three(P, pattern):
    rng = np.random.RandomState(P)
    status = {"empty": rng.choice([0, 1, 2], P), "full": np.full(P, 3), "random": rng.choice([0, 1, 2, 3], P)}[pattern].astype(np.uint8)
    state = ops.lattice_state(1, P, 1)
    state.status.copy_(torch.from_numpy(status))
    want = np.flatnonzero(status == 3)
    pix, n = ops.lattice_select(state)
    pix2, n2 = ops.lattice_select(state)                                  # the workspace is reused: the same answer again
    torch.cuda.synchronize()
    assert n == n2 == len(want) and pix.dtype == torch.int32
    assert np.array_equal(pix.cpu().numpy(), want) and np.array_equal(pix2.cpu().numpy(), want)
    assert n == {"empty": 0, "full": P}.get(pattern, n)


# ---------------------------------------------------------------------------------------- argument errors
def test_bad_arguments_are_error_codes_and_nothing_is_launched():
    h, w, K, Cw = 9, 9, 2, 11
    P = h * w
    lib, stream, null = hip.lib(), hip.stream_ptr(), C.c_void_p(0)
    values = torch.full((P, Cw), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    status = torch.zeros(P, dtype=torch.uint8, device="cuda")             # all unknown: a launch would fill or queue
    flat = torch.full((P,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    tol = torch.full((Cw - 1,), float("inf"), device="cuda")
    out = torch.full((P,), POISON, dtype=torch.int32, device="cuda")
    n_out = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    work = torch.empty(256, dtype=torch.uint8, device="cuda")
    rows = torch.zeros(4, Cw, device="cuda")
    pix = torch.arange(4, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    begin = lambda hh=h, ww=w, lv=K, st=p(status): lib.stnerf_lattice_begin(hh, ww, lv, null, st, stream)
    cls = lambda lv=K, s=4, Cc=Cw, Ee=1, nflat=P, tl=p(tol): lib.stnerf_lattice_classify(p(values), p(status), h, w, Cc, Ee, lv, s, tl, p(flat), nflat, stream)
    sel = lambda PP=P, nbytes=256, wk=p(work): lib.stnerf_lattice_select(p(status), PP, p(out), p(n_out), wk, nbytes, stream)
    sca = lambda n=4, Cc=Cw, stride=Cw, PP=P, px=p(pix): lib.stnerf_lattice_scatter(p(rows), n, Cc, stride, px, PP, p(values), p(status), stream)
    calls = [begin(hh=0), begin(lv=5), begin(lv=-1), begin(st=null), begin(hh=1 << 16, ww=1 << 16),
             cls(lv=5), cls(s=3), cls(s=8), cls(s=1), cls(lv=0, s=2), cls(Cc=0), cls(Cc=4097), cls(Ee=-1), cls(Ee=Cw + 1), cls(nflat=3), cls(tl=null),
             sel(PP=0), sel(nbytes=255), sel(wk=null),
             sca(n=-1), sca(n=P + 1), sca(stride=Cw - 1), sca(Cc=0), sca(PP=0), sca(px=null)]
    torch.cuda.synchronize()
    assert all(rc == hip.EINVAL for rc in calls), calls
    assert not bool(status.any()) and bool((bits(values) == POISON).all()) and bool((flat == POISON_BYTE).all())
    assert bool((out == POISON).all()) and int(n_out.item()) == POISON
    # the same entries with good arguments do launch
    assert begin() == hip.OK and sel() == hip.OK
    torch.cuda.synchronize()
    assert int(n_out.item()) == 9 and bool(status.any())
    with pytest.raises(ValueError, match="power of two"):
        ops.lattice_classify(ops.lattice_state(h, w, Cw), K, 3, tol)
    with pytest.raises(ValueError, match="outside 0..4"):
        ops.lattice_begin(ops.lattice_state(h, w, Cw), 5)


# ---------------------------------------------------------------------------------------- the driver
H, W = 24, 32
N = H * W
THR, BTHR, CHUNCKS = 0.05, 0.02, 64


def scene(precision):
    """The model and frame ids of tests/test_gpu_accumulate.py's driver tests, its draws the device's, a 24 x 32 camera."""
    case = OCC.plain_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids = [float(x) for x in case["groups"][0][1]]
    K, T = syn.camera(H, W, case["orbit"])
    model = SE.make_model(case, precision)
    model.replay = None
    return model, K, T, ids


def packed_of(out, l):
    """The reference 5-tuple of a "fine" frame -> (n, 6 + 5 l): the row the driver keeps per pixel."""
    fine, coarse, layers, coarse_layers, masks = out
    assert coarse is None and coarse_layers is None
    mask_bits = sum(m.to(torch.float32) * float(1 << i) for i, m in enumerate(masks)).reshape(-1, 1)
    return torch.cat(list(fine) + [x for t in layers for x in t] + [mask_bits], 1)


def assert_same_frame(a, b):
    for x, y in zip(a[0], b[0]):
        assert same_bits(x, y)
    for la, lb in zip(a[2], b[2]):
        for x, y in zip(la, lb):
            assert same_bits(x, y)
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[4]))


def render_list(model, K, T, ids, pix=None):
    """A list of the view's pixels as the op-level entries render it: seed 11, the view's thresholds."""
    model.seed = 11
    rays = ops.generate_rays(K, T, H, W, frame_ids=ids, pixels=None if pix is None else dev(pix, np.int32))
    with torch.no_grad():
        raw = model.render_rays_raw(rays, False, THR, BTHR, ref_chunk=CHUNCKS)
    return parallel.pack_outputs(raw, "fine").cpu().numpy()


def colour_columns(l):
    return [c for c in range(5 + 5 * l) if c % 5 < 3]


def median_spread(plain, K, l):
    """The median over the top-level cells of the plain frame of the corner spread of their colour columns (the largest one)."""
    spread = L.top_cell_spread(plain, H, W, K, colour_columns(l))
    assert len(spread) == 7 * 5 and np.isfinite(spread).all()
    return float(np.median(spread))


@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_levels_zero_and_a_force_of_ones_are_the_plain_frame(precision, fresh):
    model, K, T, ids = scene(precision)
    model.fresh_draws_per_call = fresh
    s0 = model.seed = 11
    plain = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, gather="fine")
    assert model.seed == (s0 + 1 if fresh else s0)
    for spec in (LatticeSpec(0, 0.0), LatticeSpec(2, 1.0, force=torch.ones(H, W, dtype=torch.uint8)), dict(levels=0, tol_rgb=9.0, force=None)):
        model.seed = s0
        out, stats = parallel.render_view_lattice(model, K, T, H, W, ids, spec, THR, BTHR, chuncks=CHUNCKS)
        torch.cuda.synchronize()
        assert model.seed == (s0 + 1 if fresh else s0)
        assert out[1] is None and out[3] is None
        assert_same_frame(plain, out)
        assert (stats["rendered"], stats["filled"]) == (N, 0) and bool((stats["status"] == 1).all())
        assert stats["rays_per_level"][0] == N and sum(stats["rays_per_level"]) == N
    # the small-call rule is the view's: with chuncks above h w the model's defaults render, as layered_batchify_ray's would
    model.seed = s0
    small = parallel.render_view(model, K, T, H, W, ids, THR, BTHR)
    model.seed = s0
    out, _ = parallel.render_view_lattice(model, K, T, H, W, ids, LatticeSpec(0, 0.0), THR, BTHR)
    assert same_bits(small[0][0], out[0][0]) and not same_bits(small[0][0], plain[0][0])


@pytest.mark.parametrize("force", [None, "performers"])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_two_levels_replay_as_the_op_level_loop(precision, force):
    """K = 2 with tol_rgb = the median corner spread of the plain frame's top-level cells: the loop is replayed here with the same
    ``generate_rays(pixels=)`` and ``render_rays_raw`` calls and the RESTATEMENT's begin, classify, select and scatter; the driver's
    values, status and rays per level must be those, bit for bit."""
    model, K, T, ids = scene(precision)
    l, Kl = model.total_layers, 2
    plain = render_list(model, K, T, ids)
    tol_rgb = median_spread(plain, Kl, l)
    assert tol_rgb > 0.0
    forced = None
    if force == "performers":
        hit = model.ray_masks(ops.generate_rays(K, T, H, W, frame_ids=ids), CHUNCKS)
        forced = (hit[:, 1:] != 0).any(1).cpu().numpy().astype(np.uint8).reshape(H, W)
        assert forced.any() and not forced.all()
    values, status, rays, counts = L.run(H, W, Kl, L.width(l), L.tolerances(l, tol_rgb), lambda pix: render_list(model, K, T, ids, pix), forced)
    print(f"{precision}, force {force}: tol_rgb {tol_rgb:.3e}, rays per level {rays}, (filled, queued) per level {counts}")
    model.seed = 11
    out, stats = parallel.render_view_lattice(model, K, T, H, W, ids, LatticeSpec(Kl, tol_rgb, force=force), THR, BTHR, chuncks=CHUNCKS)
    torch.cuda.synchronize()
    assert model.seed == 11
    assert stats["rays_per_level"] == rays and len(rays) == Kl + 1
    assert torch.equal(stats["status"], dev(status, np.uint8))
    assert torch.equal(bits(packed_of(out, l)), bits(dev(values, F)))
    n_filled = int((status == L.FILLED).sum())
    assert (stats["filled"], stats["rendered"]) == (n_filled, N - n_filled) and sum(rays) == N - n_filled
    assert 0 < stats["filled"] < N
    assert stats["margin"] == N - 29 * 21 and stats["forced"] == (0 if forced is None else int(forced.sum()))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_performers_are_never_interpolated(precision):
    """force = "performers" (the default): on every filled pixel the plain frame's returned masks have no performer bit."""
    model, K, T, ids = scene(precision)
    l = model.total_layers
    tol_rgb = median_spread(render_list(model, K, T, ids), 2, l)
    model.seed = 11
    plain = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, gather="fine")
    out, stats = parallel.render_view_lattice(model, K, T, H, W, ids, LatticeSpec(2, tol_rgb), THR, BTHR, chuncks=CHUNCKS)
    torch.cuda.synchronize()
    filled = stats["status"] == 2
    performer = torch.stack([plain[4][i] for i in range(1, l)], 1).any(1)
    assert bool(filled.any()) and bool(performer.any()) and stats["forced"] >= int(performer.sum())
    assert not bool((filled & performer).any())
    assert not bool((filled & torch.stack([out[4][i] for i in range(1, l)], 1).any(1)).any())
    # hidden performers are not forced: their pixels may be filled again
    for i in range(1, l):
        model.hide_layer(i)
    try:
        _, hidden = parallel.render_view_lattice(model, K, T, H, W, ids, LatticeSpec(2, tol_rgb), THR, BTHR, chuncks=CHUNCKS)
    finally:
        for i in range(1, l):
            model.show_layer(i)
    assert hidden["forced"] == 0 and hidden["filled"] > 0


def test_the_driver_refuses_what_contradicts_a_sparse_list():
    from stnerf_amd.bkgd_cache import BackgroundCache
    from stnerf_amd.layer_cache import LayerCache
    from stnerf_amd.occupancy import OccupancyGrids
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    spec = LatticeSpec(2, 0.05)
    call = lambda spec=spec, **kw: parallel.render_view_lattice(model, K, T, H, W, ids, spec, THR, BTHR, chuncks=CHUNCKS, **kw)
    model.set_background_cache(BackgroundCache())
    with pytest.raises(ValueError, match="sparse list"):
        call()
    model.set_background_cache(None)
    model.set_layer_cache(LayerCache())
    with pytest.raises(ValueError, match="sparse list"):
        call()
    model.set_layer_cache(None)
    model.replay = {"jitter": torch.zeros(model.total_layers, N, model.coarse_ray_sample, device="cuda")}
    with pytest.raises(ValueError, match="replay"):
        call()
    model.replay = None
    with pytest.raises(ValueError, match="out of scope"):
        call(scene=True)
    with pytest.raises(ValueError, match="out of scope"):
        call(occluder=torch.zeros(N, 5, device="cuda"))
    with pytest.raises(ValueError, match="accumulate= or reproject="):
        call(accumulate=dict(max_spp=2))
    with pytest.raises(ValueError, match="aperture"):
        call(lens=dict(aperture=0.05, focus=3.0))
    with pytest.raises(ValueError, match=r"\(24,32\)"):
        call(LatticeSpec(2, 0.05, force=torch.ones(W, H, dtype=torch.uint8)))
    pairs = list(enumerate(ids))
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(model, T, K, H, W, pairs, 20.0, lattice=spec, scene_passes=True)
    assert model.seed == 11
    # occupancy grids act inside the render call as always; a distorting lens passes through
    model.set_occupancy(OccupancyGrids(res=16))
    out, stats = call()
    assert stats["rendered"] + stats["filled"] == N
    model.set_occupancy(None)
    out, stats = call(lens=dict(k1=0.05))
    assert stats["rendered"] + stats["filled"] == N
    torch.cuda.synchronize()


def test_render_pose_and_the_renderer_return_the_drivers_frame():
    from stnerf_amd.render import LayeredNeuralRenderer
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    l, far = model.total_layers, 20.0
    tol_rgb = median_spread(render_list(model, K, T, ids), 2, l)
    spec = LatticeSpec(2, tol_rgb)
    pairs = list(enumerate(ids))
    model.seed = 11
    color, depth, color_layer, depth_layer, stats = render_pose(model, T, K, H, W, pairs, far, THR, BTHR, lattice=spec)
    out, flat = parallel.render_view_lattice(model, K, T, H, W, ids, spec, THR, BTHR)
    assert same_bits(color, out[0][0].reshape(H, W, 3)) and same_bits(depth, out[0][1].reshape(H, W, 1).clamp_min(0) / far)
    for i in range(l):
        assert same_bits(color_layer[i], out[2][i][0].reshape(H, W, 3)) and same_bits(depth_layer[i], out[2][i][1].reshape(H, W, 1) / far)
    assert stats["status"].shape == (H, W) and torch.equal(stats["status"].reshape(-1), flat["status"])
    assert all(stats[k] == flat[k] for k in ("rendered", "filled", "forced", "margin", "rays_per_level")) and 0 < stats["filled"] < N
    # the renderer over a 2-pose path
    K2, T2 = syn.camera(H, W, 40.0)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    seen = []

    def on_frame(idx, c, d, cl, dl, lattice=None):
        seen.append((idx, c.clone(), d.clone(), [x.clone() for x in cl], lattice))

    for flip in (False, True):
        seen.clear()
        r = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.stack([torch.as_tensor(T), torch.as_tensor(T2)]), gt_Ks=[K, K2],
                                  lattice=dict(levels=2, tol_rgb=tol_rgb))
        r.set_path_gt_poses()
        assert len(r.poses) == 2 and isinstance(r.lattice, LatticeSpec)
        r.render_path(inverse_y_axis=flip, on_frame=on_frame)
        assert len(seen) == 2 and len(r.lattice_stats) == 2 and len(r.images) == 2
        for k in range(2):
            c, d, cl, dl, st = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0, lattice=r.lattice)
            turn = (lambda x: torch.flip(x, [0])) if flip else (lambda x: x)
            idx, sc, sd, scl, lat = seen[k]
            assert idx == k and same_bits(sc, turn(c)) and same_bits(sd, turn(d)) and all(same_bits(a, turn(b)) for a, b in zip(scl, cl))
            assert lat is not None and torch.equal(lat["status"], turn(st["status"])) and lat["rays_per_level"] == st["rays_per_level"]
            assert r.lattice_stats[k] == {key: v for key, v in st.items() if key != "status"}
    # without lattice= nothing changes: no keyword, no stats
    plain = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.as_tensor(T)[None], gt_Ks=[K])
    plain.set_path_gt_poses()
    plain.render_path(on_frame=lambda idx, c, d, cl, dl: None)
    assert plain.lattice is None and plain.lattice_stats == []
    torch.cuda.synchronize()
