"""Progressive multi-sample frames on the MI355X (csrc/accumulate.hip): the ray generator over a pixel
list, the Welford scatter-accumulator and the ordered compaction against the numpy oracle of tests/accumulate_common.py, bit for
bit; then the driver (``parallel.render_view_accumulated``), ``render_pose(accumulate=)`` and the renderer's ``accumulate=``
on the small model and camera of tests/test_gpu_occluder.py::test_render_pose_with_an_occluder (17 x 23 = 391 rays)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import accumulate_common as A
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import bits, detach_models, same_bits
from stnerf_amd import hip, ops, parallel, synthetic as syn
from stnerf_amd.accumulate import AccumulateSpec

pytestmark = pytest.mark.gpu

F = np.float32
H, W = S.H, S.W                 # 17 x 23
N = H * W
POISON = 0x7FC0BEEF             # a NaN pattern no kernel writes
IDS3 = [1.0, 2.5, 3.0]


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def camera():
    K, T = syn.camera(H, W, 15.0)
    return K, T, torch.inverse(K.to(torch.float32)).numpy(), torch.as_tensor(T, dtype=torch.float32).numpy()


# ---------------------------------------------------------------------------------------- rays of a pixel list
def pixel_list(n, order):
    pix = np.random.RandomState(100 + n).choice(N, n, replace=False)
    return np.sort(pix) if order == "ascending" else pix


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 391])
def test_listed_rays_with_zero_offset_are_the_plain_rows(n, order):
    K, T, _, _ = camera()
    plain = ops.generate_rays(K, T, H, W, frame_ids=IDS3)
    pix = pixel_list(n, order)
    rays = ops.generate_rays(K, T, H, W, frame_ids=IDS3, pixels=dev_i32(pix))
    torch.cuda.synchronize()
    assert rays.shape == (n, 9) and same_bits(rays, plain[torch.from_numpy(pix).cuda().long()])


def raw_generate(pixels, n, du, dv, rows=None, fids=IDS3):
    """stnerf_generate_rays_list itself, on a poisoned buffer of ``rows`` >= n rows."""
    K, T, kinv, Tm = camera()
    rows = n if rows is None else rows
    out = torch.full((rows, 6 + len(fids)), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    kin, tin, fin = (C.c_float * 9)(*kinv.reshape(-1).tolist()), (C.c_float * 16)(*Tm.reshape(-1).tolist()), (C.c_float * len(fids))(*fids)
    rc = hip.lib().stnerf_generate_rays_list(kin, tin, H, W, hip.dptr(pixels, torch.int32), n, du, dv, fin, len(fids), hip.dptr(out),
                                             out.shape[1], hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("n", [1, 65, 391])
def test_a_null_list_is_the_contiguous_pixels(n):
    K, T, _, _ = camera()
    plain = ops.generate_rays(K, T, H, W, frame_ids=IDS3)
    rc, out = raw_generate(None, n, 0.0, 0.0, rows=n + 3)
    assert rc == hip.OK and same_bits(out[:n], plain[:n])
    assert bool((bits(out[n:]) == POISON).all())                       # nothing beyond row n - 1


@pytest.mark.parametrize("p", [1, 2, 3, 7])
def test_offset_rays_equal_the_numpy_restatement(p):
    K, T, kinv, Tm = camera()
    du, dv = (float(x) for x in A.offset(p))
    assert (du, dv) != (0.0, 0.0)
    for pix in (None, pixel_list(65, "shuffled"), pixel_list(391, "ascending")):
        n = N if pix is None else len(pix)
        rays = ops.generate_rays(K, T, H, W, frame_ids=IDS3, offset=(du, dv), pixels=None if pix is None else dev_i32(pix)).cpu().numpy()
        want = A.rays_of_pixels(kinv, Tm, W, np.arange(N) if pix is None else pix, du, dv, IDS3)
        print(f"pass {p}, {'no list' if pix is None else len(pix)}: max |difference| = {np.abs(rays - want).max():.3e}")
        assert rays.shape == (n, 9) and A.same_bits(rays, want)
    # and the offset moves the rays: pass p is not the plain view
    assert not np.array_equal(rays[:, 3:6], ops.generate_rays(K, T, H, W, frame_ids=IDS3).cpu().numpy()[:, 3:6])


def test_a_list_entry_outside_the_view_is_skipped_and_bad_arguments_are_error_codes():
    pix = np.array([5, -1, 390, 391, 7, 1 << 30], np.int32)
    rc, out = raw_generate(dev_i32(pix), len(pix), 0.25, -0.25)
    assert rc == hip.OK
    written = ~(bits(out) == POISON).all(1).cpu().numpy()
    assert written.tolist() == [True, False, True, False, True, False]
    _, _, kinv, Tm = camera()
    assert A.same_bits(out.cpu().numpy()[written], A.rays_of_pixels(kinv, Tm, W, pix[written], 0.25, -0.25, IDS3))
    # what the host can prove wrong is an error code before any launch (the buffer stays poisoned)
    for n, du, fids in ((N + 1, 0.0, IDS3), (-1, 0.0, IDS3), (4, float("nan"), IDS3), (4, 0.0, [0.0] * 18)):
        rc, out = raw_generate(None, n, du, 0.0, rows=8, fids=fids)
        assert rc == hip.EINVAL and bool((bits(out) == POISON).all()), (n, du, len(fids))
    with pytest.raises(ValueError, match="at most once"):
        ops.generate_rays(*camera()[:2], H, W, pixels=torch.zeros(N + 1, dtype=torch.int32, device="cuda"))
    state = ops.accumulate_state(10, 10)
    with pytest.raises(ValueError, match="at most once"):
        ops.accumulate(torch.zeros(11, 10, device="cuda"), state)
    with pytest.raises(ValueError, match="floats wide"):
        ops.accumulate(torch.zeros(10, 11, device="cuda"), state)
    with pytest.raises(ValueError, match="spp range"):
        ops.accumulate_select(state, 3, 2, 0.0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- the accumulator
@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("Cw", [10, 20])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_accumulate_equals_the_oracle_bit_for_bit(n, Cw, pad, listed):
    """Four successive updates of n rows (row stride Cw + pad) into P = n + 37 pixels: without a list rows 0..n-1, with one a
    fresh shuffled subset of the first n + 30 every time, so pixels sit at different counts and the untouched ones must keep their state.  The first
    update carries a -0.0 and a large-magnitude column (whose second moment overflows, as the oracle's does)."""
    rng = np.random.RandomState(n * 7 + Cw + pad)
    P = n + 37
    state, want = ops.accumulate_state(P, Cw, 3), A.State(P, Cw, 3)
    for k in range(4):
        buf = rng.randn(n, Cw + pad).astype(F)
        if k == 0:
            buf[:, 0] = -0.0
            buf[:, 1] = F(1e30)
            buf[::2, 4] = F(-3e38)
        pix = rng.choice(P - 7, n, replace=False).astype(np.int32) if listed else None      # (the last 7 pixels: never named)
        values = torch.from_numpy(buf).cuda()[:, :Cw]
        assert values.stride(0) == Cw + pad or n == 1
        ops.accumulate(values, state, None if pix is None else dev_i32(pix))
        A.update(want, buf[:, :Cw], pix)
        torch.cuda.synchronize()
        assert np.array_equal(state.count.cpu().numpy(), want.count), k
        assert A.same_bits(state.mean.cpu().numpy(), want.mean), k
        assert A.same_bits(state.m2.cpu().numpy(), want.m2), k
    assert (want.count == 0).any() and want.count.max() >= 1                   # untouched pixels beside updated ones
    assert listed or (want.count[:n] == 4).all()


# ---------------------------------------------------------------------------------------- the pixels still active
MIN_SPP, MAX_SPP, TOL = 3, 6, 0.125


def select_state(P, pattern):
    """count and m2 of P pixels in a pattern, as numpy; the rule's own edge in "straddle": counts min - 1, min, max - 1, max and
    one m2 column exactly at, just above or just below tol2 * (float)(c (c - 1))."""
    q = np.arange(P)
    m2 = np.zeros((P, 3), F)
    if pattern == "all":
        count = np.zeros(P, np.int32)
    elif pattern == "none":
        count = np.full(P, MAX_SPP, np.int32)
        m2[:] = F(1e6)                                       # noisy, but at max_spp
    elif pattern == "alternating":
        count = np.where(q % 2 == 0, MIN_SPP - 1, MAX_SPP).astype(np.int32)
    elif pattern == "last":
        count = np.full(P, MIN_SPP, np.int32)                # quiet (m2 = 0) and past min_spp: stopped
        count[-1] = MIN_SPP - 1
    else:
        rng = np.random.RandomState(P % 1000)
        count = rng.choice([MIN_SPP - 1, MIN_SPP, MAX_SPP - 1, MAX_SPP], P).astype(np.int32)
        bound = A.tol_squared(TOL) * (count * (count - 1)).astype(F)
        edge = rng.randint(0, 4, P)                          # 0: at the bound, 1: one ulp above, 2: one ulp below, 3: NaN
        value = np.where(edge == 0, bound, np.where(edge == 1, np.nextafter(bound, F(np.inf)), np.nextafter(bound, F(-np.inf)))).astype(F)
        value[edge == 3] = np.nan
        m2[q, rng.randint(0, 3, P)] = value
    return count, m2


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "last", "straddle"])
@pytest.mark.parametrize("P", [1, 64, 255, 256, 257, 70001, 262145])
def test_select_equals_flatnonzero_of_the_oracles_rule(P, pattern):
    count, m2 = select_state(P, pattern)
    want = A.State(P, 3, 3)
    want.count, want.m2 = count, m2
    state = ops.accumulate_state(P, 3, 3)
    state.count.copy_(torch.from_numpy(count))
    state.m2.copy_(torch.from_numpy(m2))
    expect = A.select(want, MIN_SPP, MAX_SPP, TOL)
    pixels, n = ops.accumulate_select(state, MIN_SPP, MAX_SPP, TOL)
    pixels2, n2 = ops.accumulate_select(state, MIN_SPP, MAX_SPP, TOL)      # the workspace is reused: the same answer again
    torch.cuda.synchronize()
    assert n == n2 == len(expect) and pixels.dtype == torch.int32
    assert np.array_equal(pixels.cpu().numpy(), expect) and np.array_equal(pixels2.cpu().numpy(), expect)
    if pattern == "all":
        assert n == P
    if pattern == "none":
        assert n == 0
    if pattern == "last":
        assert expect.tolist() == [P - 1]
    if pattern == "straddle" and P >= 255:
        act = A.active(want, MIN_SPP, MAX_SPP, TOL)
        assert act.any() and not act.all()


# ---------------------------------------------------------------------------------------- the driver
THR, BTHR, CHUNCKS = 0.05, 0.02, 64


def scene(precision):
    """The model, camera and frame ids of tests/test_gpu_occluder.py::test_render_pose_with_an_occluder, its draws the device's."""
    case = OCC.plain_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids = [float(x) for x in case["groups"][0][1]]
    K, T = syn.camera(S.H, S.W, case["orbit"])
    model = SE.make_model(case, precision)
    model.replay = None
    return model, K, T, ids


def means_of(out):
    """The reference 5-tuple -> (n, 5 + 5 l): the row the driver accumulates."""
    fine, coarse, layers, coarse_layers, masks = out
    assert coarse is None and coarse_layers is None
    return torch.cat(list(fine) + [x for t in layers for x in t], 1)


def render_pass(model, K, T, ids, s0, p, shutters, pix=None):
    """Pass p as the op-level entries render it: the schedule's offset and frame ids, seed s0 + p, the view's thresholds."""
    model.seed = s0 + p
    rays = ops.generate_rays(K, T, H, W, frame_ids=[float(x) for x in A.layer_frame_ids(p, ids, shutters)],
                             offset=tuple(float(x) for x in A.offset(p)), pixels=None if pix is None else dev_i32(pix))
    with torch.no_grad():
        raw = model.render_rays_raw(rays, False, THR, BTHR, ref_chunk=CHUNCKS)
    return parallel.pack_outputs(raw, "fine")[:, :-1].cpu().numpy()


@pytest.mark.parametrize("fresh", [False, True])
@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_one_pass_is_the_plain_frame(precision, fresh):
    model, K, T, ids = scene(precision)
    model.fresh_draws_per_call = fresh
    s0 = model.seed = 11
    plain = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS)
    assert model.seed == (s0 + 1 if fresh else s0)
    model.seed = s0
    out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(1), THR, BTHR, chuncks=CHUNCKS)
    torch.cuda.synchronize()
    assert model.seed == (s0 + 1 if fresh else s0)
    for a, b in zip(plain[0], out[0]):
        assert same_bits(a, b)
    for la, lb in zip(plain[2], out[2]):
        for a, b in zip(la, lb):
            assert same_bits(a, b)
    assert all(torch.equal(a, b) for a, b in zip(plain[4], out[4])) and out[1] is None and out[3] is None
    assert stats["passes"] == 1 and stats["rays_rendered"] == N and bool((stats["spp"] == 1).all()) and not bool(stats["variance"].any())
    # the small-call rule is the view's: with chuncks above h w the model's defaults render, as layered_batchify_ray's would
    model.seed = s0
    small = parallel.render_view(model, K, T, H, W, ids, THR, BTHR)
    model.seed = s0
    out, _ = parallel.render_view_accumulated(model, K, T, H, W, ids, dict(max_spp=1), THR, BTHR)
    assert same_bits(small[0][0], out[0][0]) and not same_bits(small[0][0], plain[0][0])


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_fixed_spp_is_the_oracles_mean_of_separately_rendered_passes(precision):
    model, K, T, ids = scene(precision)
    l = model.total_layers
    shutters = [0.0, 0.8] + [0.0] * (l - 2)                             # motion blur on performer 1 alone
    s0 = 11
    want = A.State(N, 5 + 5 * l, 3)
    rows = []
    for p in range(3):
        rows.append(render_pass(model, K, T, ids, s0, p, shutters))
        A.update(want, rows[-1])
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    model.seed = s0
    out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(3, shutter=shutters), THR, BTHR, chuncks=CHUNCKS)
    torch.cuda.synchronize()
    assert model.seed == s0
    assert A.same_bits(means_of(out).cpu().numpy(), want.mean)
    assert bool((stats["spp"] == 3).all()) and stats["passes"] == 3 and stats["rays_rendered"] == 3 * N
    assert stats["spp"].dtype == torch.int32 and stats["spp"].shape == (N,) and stats["variance"].shape == (N, 3)
    # the reported variance of the mean: m2 / (c (c - 1)), c (c - 1) = 6 exactly, one rounding of the quotient (2^-22 allows a
    # quotient that is faithfully rather than correctly rounded)
    assert np.allclose(stats["variance"].cpu().numpy(), A.variance_of_mean(want), rtol=2.0 ** -22, atol=0.0)
    # the scalar shutter reaches every performer: another frame than the one above
    model.seed = s0
    other, _ = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(3, shutter=0.8, frame_range=(1.0, 3.0)), THR, BTHR,
                                                chuncks=CHUNCKS)
    assert not same_bits(means_of(other), means_of(out))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_adaptive_spp_replays_as_the_op_level_loop(precision):
    """(min 2, max 4), tol = the median over the pixels of the oracle's standard error after two passes (the largest of the three
    colour channels): about half the pixels stop at 2.  The loop is replayed here with the op-level entries and the ORACLE's
    update and select; the driver's means, spp map, pass count and ray count must be those, bit for bit."""
    model, K, T, ids = scene(precision)
    l = model.total_layers
    shutters = [0.0, 0.8] + [0.0] * (l - 2)
    s0 = 11
    want = A.State(N, 5 + 5 * l, 3)
    for p in range(2):
        A.update(want, render_pass(model, K, T, ids, s0, p, shutters))
    tol = float(np.median(np.sqrt(A.variance_of_mean(want)).max(1)))
    assert tol > 0.0
    passes, rendered, lists = 2, 2 * N, []
    while passes < 4:
        pix = A.select(want, 2, 4, tol)
        if len(pix) == 0:
            break
        lists.append(pix)
        A.update(want, render_pass(model, K, T, ids, s0, passes, shutters, pix), pix)
        rendered += len(pix)
        passes += 1
    print(f"{precision}: tol {tol:.3e}, lists {[len(x) for x in lists]}, spp histogram {np.bincount(want.count).tolist()}")
    model.seed = s0
    model.fresh_draws_per_call = True
    out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(4, 2, tol, shutter=shutters), THR, BTHR,
                                                  chuncks=CHUNCKS)
    torch.cuda.synchronize()
    assert model.seed == s0 + passes
    assert stats["passes"] == passes and stats["rays_rendered"] == rendered
    assert np.array_equal(stats["spp"].cpu().numpy(), want.count)
    assert A.same_bits(means_of(out).cpu().numpy(), want.mean)
    assert (want.count == 2).any() and (want.count == 4).any()            # not vacuous: some pixel stopped, some ran to the end
    assert 0.25 * N <= (want.count == 2).sum() <= 0.75 * N               # "roughly half"


def test_the_driver_refuses_what_it_cannot_average():
    from stnerf_amd.bkgd_cache import BackgroundCache
    from stnerf_amd.layer_cache import LayerCache
    from stnerf_amd.occupancy import OccupancyGrids
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    call = lambda spec, **kw: parallel.render_view_accumulated(model, K, T, H, W, ids, spec, THR, BTHR, chuncks=CHUNCKS, **kw)
    model.set_background_cache(BackgroundCache())
    with pytest.raises(ValueError, match="one jitter pattern"):
        call(AccumulateSpec(2))
    model.set_background_cache(None)
    model.set_layer_cache(LayerCache())
    with pytest.raises(ValueError, match="one jitter pattern"):
        call(AccumulateSpec(2))
    model.set_layer_cache(None)
    model.set_occupancy(OccupancyGrids(res=16))
    with pytest.raises(ValueError, match="keyed by frame"):
        call(AccumulateSpec(2, shutter=0.5))
    out, stats = call(AccumulateSpec(2))                                 # grids with shutter 0 need nothing: model state
    assert stats["passes"] == 2
    model.set_occupancy(None)
    pairs = list(enumerate(ids))
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(model, T, K, H, W, pairs, 20.0, accumulate=AccumulateSpec(2), scene_passes=True)
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(model, T, K, H, W, pairs, 20.0, accumulate=AccumulateSpec(2), occluder=(torch.zeros(H, W, 4), torch.ones(H, W)))
    assert model.seed == 11
    torch.cuda.synchronize()


def test_render_pose_and_the_renderer_accumulate():
    from stnerf_amd.render import LayeredNeuralRenderer
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    l, far = model.total_layers, 20.0
    # tol: the median standard error after two passes of this view, so that about half its pixels take the third
    _, two = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(2, shutter=0.5, frame_range=(1.0, 3.0)), THR, BTHR)
    tol = float(two["variance"].max(1)[0].sqrt().median())
    spec = AccumulateSpec(3, 2, tol, shutter=0.5, frame_range=(1.0, 3.0))
    # render_pose: the driver's means with the reference's depth post-processing, stats as images
    pairs = list(enumerate(ids))
    color, depth, color_layer, depth_layer, stats = render_pose(model, T, K, H, W, pairs, far, THR, BTHR, accumulate=spec)
    out, flat = parallel.render_view_accumulated(model, K, T, H, W, ids, spec, THR, BTHR)
    assert same_bits(color, out[0][0].reshape(H, W, 3)) and same_bits(depth, out[0][1].reshape(H, W, 1).clamp_min(0) / far)
    for i in range(l):
        assert same_bits(color_layer[i], out[2][i][0].reshape(H, W, 3)) and same_bits(depth_layer[i], out[2][i][1].reshape(H, W, 1) / far)
    assert stats["spp"].shape == (H, W) and torch.equal(stats["spp"].reshape(-1), flat["spp"])
    assert stats["variance"].shape == (H, W, 3) and (stats["passes"], stats["rays_rendered"]) == (flat["passes"], flat["rays_rendered"])
    assert 2 <= int(stats["spp"].min()) and int(stats["spp"].max()) == 3 and N * 2 < stats["rays_rendered"] < N * 3
    # the renderer over a 2-pose path
    K2, T2 = syn.camera(H, W, 40.0)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    seen = []

    def on_frame(idx, c, d, cl, dl, accumulated=None):
        seen.append((idx, c.clone(), d.clone(), [x.clone() for x in cl], accumulated))

    for flip in (False, True):
        seen.clear()
        r = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.stack([torch.as_tensor(T), torch.as_tensor(T2)]), gt_Ks=[K, K2],
                                  accumulate=dict(max_spp=3, min_spp=2, tol=tol, shutter=0.5, frame_range=(1.0, 3.0)))
        r.set_path_gt_poses()
        assert len(r.poses) == 2 and isinstance(r.accumulate, AccumulateSpec)
        r.render_path(inverse_y_axis=flip, on_frame=on_frame)
        assert len(seen) == 2 and len(r.spp_maps) == 2 and len(r.images) == 2
        for k in range(2):
            c, d, cl, dl, st = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0, accumulate=r.accumulate)
            turn = (lambda x: torch.flip(x, [0])) if flip else (lambda x: x)
            idx, sc, sd, scl, acc = seen[k]
            assert idx == k and same_bits(sc, turn(c)) and same_bits(sd, turn(d)) and all(same_bits(a, turn(b)) for a, b in zip(scl, cl))
            assert acc is not None and torch.equal(acc["spp"], turn(st["spp"])) and same_bits(acc["variance"], turn(st["variance"]))
            assert acc["passes"] == st["passes"] and acc["rays_rendered"] == st["rays_rendered"]
            assert torch.equal(r.spp_maps[k], turn(st["spp"]).cpu()) and r.spp_maps[k].shape == (H, W)
            assert k or not torch.equal(st["spp"], torch.flip(st["spp"], [0]))     # (frame 0's is a map that a flip changes)
    r.render_path_walking(auto_save=True, on_frame=on_frame)
    assert len(r.spp_maps) == 2 and len(seen) == 4 and seen[-1][4] is not None
    # without accumulate= nothing changes: no keyword, no maps
    plain = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.as_tensor(T)[None], gt_Ks=[K])
    plain.set_path_gt_poses()
    plain.render_path(on_frame=lambda idx, c, d, cl, dl: None)
    assert plain.accumulate is None and plain.spp_maps == []
    torch.cuda.synchronize()
