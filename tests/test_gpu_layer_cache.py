"""The layer cache (stnerf_amd.LayerCache, stnerf_render_rays_layers, stnerf_copy_layer_raw_listed): from a fixed view a performer
whose own inputs did not change is copied in instead of evaluated.  A frame rendered from the cache must be bit-identical to the
frame rendered without one; a layer must hit when only other layers, opacities, thresholds or shown flags changed and miss when one
of its own inputs did.  Shapes: views of 23 x 17 = 391 rays (no multiple of 64 or 128) in launch pieces of 128 (four pieces, the
last of 7 rays) at (n1, n2) = (8, 8) and (64, 64); the listed copy at n in {1, 17, 300}, l in {2, 4}, ns in {3, 64, 192}."""
import types

import numpy as np
import pytest
import torch

import stnerf_amd
from layer_cache_common import check_listed_copy_argument_errors, listed_copy_reference, ray_lists
from stnerf_amd import ops, parallel, synthetic as syn
from stnerf_amd.bkgd_cache import view_frame_ids, view_key
from stnerf_amd.layer_cache import CAPTURE, OFF, REUSE, entry_bytes

pytestmark = pytest.mark.gpu

H, W, CAP, CHUNK = 17, 23, 128, 64
PIECES = (H * W + CAP - 1) // CAP
SAMPLES = [(8, 8), (64, 64)]


# ---- 1. the listed copy against the numpy restatement, between canaries -----------------------------------------------------
GUARD = 256                                   # words
PATTERN = 0x7FC00A5A


def guarded(shape, dtype=torch.float32):
    numel = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((numel + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + numel].view(dtype).reshape(shape)


def intact(buf):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy()


@pytest.mark.parametrize("n", [1, 17, 300])
def test_listed_copy_is_the_numpy_restatement(n):
    rs = np.random.RandomState(n)
    cases = 0
    for l in (2, 4):
        for layer in sorted({1, l - 1}):
            for ns in (3, 64, 192):
                raw_host = rs.standard_normal((n, l, ns, 4)).astype(np.float32)
                raw_buf, raw = guarded((n, l, ns, 4))
                raw.copy_(torch.from_numpy(raw_host))
                for name, lst in ray_lists(n, rs):
                    c = len(lst)
                    padded = np.concatenate([lst, np.full(n - c, -7, np.int32)])          # (the frame's list is n wide)
                    ray_list, ray_count = torch.from_numpy(padded).cuda(), torch.tensor([c], dtype=torch.int32, device="cuda")
                    for capacity in sorted({c, c + 5, c - 1} - {-1}):
                        what = (n, l, layer, ns, name, capacity)
                        dense_buf, dense = guarded((capacity, ns, 4))
                        rays_buf, rays = guarded((capacity,), torch.int32)
                        count = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
                        before = (raw_host, np.full((capacity, ns, 4), np.float32(7.25)), np.full(capacity, 77, np.int32))
                        dense.fill_(7.25)
                        rays.fill_(77)
                        # capture
                        assert ops.copy_layer_raw_listed(raw, layer, dense, rays, count, True, ray_list=ray_list, ray_count=ray_count) is dense
                        w_raw, w_dense, w_rays, w_count, _ = listed_copy_reference(before[0], layer, before[1], before[2], 12345, True, padded, c)
                        assert int(count) == w_count == (c if c <= capacity else -1), what
                        assert np.array_equal(bits(dense), w_dense.view(np.int32)) and np.array_equal(bits(rays), w_rays), what
                        assert np.array_equal(bits(raw), raw_host.view(np.int32)), what
                        if c > capacity:                  # nothing but the count was written
                            assert np.array_equal(bits(dense), before[1].view(np.int32)) and np.array_equal(bits(rays), before[2]), what
                        # restore into another raw: only the listed rays' slice of `layer` changes; the counter accumulates
                        back_host = rs.standard_normal((n, l, ns, 4)).astype(np.float32)
                        back_buf, back = guarded((n, l, ns, 4))
                        back.copy_(torch.from_numpy(back_host))
                        mismatch = torch.tensor([5], dtype=torch.int64, device="cuda")
                        frame = torch.tensor([c + 1], dtype=torch.int32, device="cuda")    # (another hit count than the entry's)
                        assert ops.copy_layer_raw_listed(back, layer, dense, rays, count, False, ray_count=frame, mismatch=mismatch) is back
                        w_back, _, _, _, w_mis = listed_copy_reference(back_host, layer, w_dense, w_rays, w_count, False, None, c + 1, 5)
                        assert np.array_equal(bits(back), w_back.view(np.int32)), what
                        assert int(mismatch) == w_mis == (6 if w_count != c + 1 else 5), what
                        ops.copy_layer_raw_listed(back, layer, dense, rays, count, False, ray_count=count, mismatch=mismatch)
                        ops.copy_layer_raw_listed(back, layer, dense, rays, count, False)          # (no counter, no frame count)
                        assert int(mismatch) == w_mis and np.array_equal(bits(back), w_back.view(np.int32)), what
                        if 0 < c <= capacity:
                            outside = np.ones((n, l), bool)
                            outside[lst, layer] = False
                            assert np.array_equal(bits(back)[outside], back_host.view(np.int32)[outside]), what
                            assert np.array_equal(bits(back)[lst, layer], raw_host.view(np.int32)[lst, layer]), what
                        assert intact(dense_buf) and intact(rays_buf) and intact(back_buf) and intact(raw_buf), what
                        cases += 1
                    # a second slice captured under the kept list (list and count alias the entry's): both stay as they are
                    if c:
                        dense2_buf, dense2 = guarded((c, ns, 4))
                        rays2, count2 = torch.from_numpy(lst.copy()).cuda(), torch.tensor([c], dtype=torch.int32, device="cuda")
                        ops.copy_layer_raw_listed(raw, layer, dense2, rays2, count2, True, ray_list=rays2, ray_count=count2)
                        assert int(count2) == c and np.array_equal(bits(rays2), lst) and intact(dense2_buf)
                        assert np.array_equal(bits(dense2), raw_host.view(np.int32)[lst, layer])
    assert cases >= 2 * 3 * 3 * 2


def test_listed_copy_argument_errors():
    assert check_listed_copy_argument_errors() >= 12
    raw, dense = torch.zeros(4, 3, 2, 4, device="cuda"), torch.zeros(4, 2, 4, device="cuda")
    rays, count = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="not a performer"):
        ops.copy_layer_raw_listed(raw, 0, dense, rays, count, False)
    with pytest.raises(ValueError, match="a capture needs"):
        ops.copy_layer_raw_listed(raw, 1, dense, rays, count, True)
    with pytest.raises(ValueError, match="raw must be"):
        ops.copy_layer_raw_listed(raw, 1, dense[:, :1], rays, count, False)


# ---- the models and the render of the frame tests ---------------------------------------------------------------------------
def build(L):
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=8, FINE_RAY_SAMPLING=8)
    cfg = types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L))
    model = build_layered_model(cfg, camera_num=1)
    # (sigma_bias 4: at the default 0.5 the coarse SpaceNets of these seeds' performers are negative in their whole box -- empty
    # layers, on which every cache test would pass whatever the cache held.  At 4 layer 1's coarse densities straddle zero, a
    # third of its box positive, and its fine ones are positive.)
    model.load_state_dict(syn.make_state_dict(L, True, True, seed=3, sigma_bias=4.0))
    return model.cuda().eval()


_MODELS = {}


def make_model(L=2, n1=8, n2=8, precision="bf16x3", schedule="stage", background_cache=False):
    """A model in a known state (the networks are built and uploaded once per layer count) with a fresh layer cache attached."""
    if L not in _MODELS:
        _MODELS[L] = build(L)
    model = _MODELS[L]
    model.clear_instances()
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.coarse_ray_sample, model.fine_ray_sample = n1, n2
    model.set_precision(precision)
    model.mlp_schedule = schedule
    model.max_rays_per_launch = CAP
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale = model.shift = model.rotation = model.layer_alpha = None
    model.near, model.alpha = 0, 1
    for i in range(L + 1):
        model.show_layer(i)
    model.set_occupancy(None)
    model.set_termination(None)
    model.set_background_cache(stnerf_amd.BackgroundCache() if background_cache else None)
    model.set_layer_cache(stnerf_amd.LayerCache())
    return model


def render(model, K, T, frame_ids, only_coarse=False, thr=0.0, bthr=0.0, scene=False, profile=False):
    """The library outputs of the view (five tensors, six with the scene passes), rendered as parallel.render_view_share renders a
    rank's rays: generated on the device, the view key and the host frame ids set around the call."""
    rays = ops.generate_rays(K, T, H, W, frame_ids=frame_ids)
    keyed = model._bkgd_cache is not None or model._layer_cache is not None
    model.view_key = view_key(K, T, H, W, frame_ids) if keyed else None
    model.view_frame_ids = view_frame_ids(frame_ids) if keyed else None
    try:
        if profile:
            ops.profile_begin()
        with torch.no_grad():
            out = model._render_rays_raw(rays, only_coarse, thr, bthr, CHUNK, scene=scene)
        torch.cuda.synchronize()
        recs = ops.profile_end() if profile else None
    finally:
        model.view_key = model.view_frame_ids = None
    out = [o.clone() for o in out]
    return (out, recs) if profile else out


def uncached(model, *a, **kw):
    """The same frame from the model without any cache."""
    held = model._bkgd_cache, model._layer_cache
    model.set_background_cache(None)
    model.set_layer_cache(None)
    try:
        return render(model, *a, **kw)
    finally:
        model.set_background_cache(held[0])
        model.set_layer_cache(held[1])


def assert_bit_equal(got, ref, what=""):
    assert len(got) == len(ref) and len(got) in (5, 6), what
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert torch.equal(a, b), f"{what}: output {k}: {(a != b).sum().item()} elements differ"
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{what}: output {k} differs in its bits"


def recorded(cache):
    """Record what ``cache.plan`` answers, per call: (layer, mode)."""
    calls, plan = [], cache.plan

    def spy(key, *a, **kw):
        mode, entry = plan(key, *a, **kw)
        calls.append((key[0][1], mode))
        return mode, entry
    cache.plan = spy
    return calls


def fids(retiming, L, performers=(2.5, 3.0, 1.5, 2.0)):
    return [1.0] + list(performers[:L]) if retiming else [2.0]


# ---- 2. frame 3 of a key is bit-identical to the frame of a model without a cache ----------------------------------------------
def _third_frame_case(n1, n2, L=2, precision="bf16x3", schedule="stage", only_coarse=False, retiming=True, setup=None,
                      reference_setup=None, scene=False, background_cache=False, layers=None):
    model = make_model(L, n1, n2, precision, schedule, background_cache)
    if setup is not None:
        setup(model)
    l = model.total_layers
    K, T = syn.camera(H, W, 15.0)
    f = fids(retiming, l - 1)
    kw = dict(only_coarse=only_coarse, scene=scene)
    calls = recorded(model._layer_cache)
    frames = [render(model, K, T, f, **kw) for _ in range(3)]
    cached = list(range(1, l)) if layers is None else layers
    want = [OFF] * PIECES + [CAPTURE] * PIECES + [REUSE] * PIECES
    for i in cached:
        assert [m for j, m in calls if j == i] == want, (i, calls)
    st = model._layer_cache.stats(mismatch=True)
    assert st == dict(hits=PIECES * len(cached), misses=2 * PIECES * len(cached), sightings=PIECES * len(cached),
                      captures=PIECES * len(cached), skipped_over_budget=0, mismatch=0), st
    if reference_setup is not None:
        reference_setup(model)
    ref = uncached(model, K, T, f, **kw)
    for k, frame in enumerate(frames):
        assert_bit_equal(frame, ref, f"frame {k + 1}")
    assert ref[4][:, 1:].any(), "no performer ray was hit: the case shows nothing"
    return model


@pytest.mark.parametrize("n1,n2", SAMPLES)
@pytest.mark.parametrize("L", [1, 2, 3])
def test_third_frame_is_bit_identical_layers(n1, n2, L):
    model = _third_frame_case(n1, n2, L=L)
    # what an entry holds: 16 (2 n1 + n2) + 4 bytes per hit ray, against the dense figure
    held = model._layer_cache.held()
    assert len(held) == L * PIECES and all(hits is not None and capacity == max(hits, 1) for _, capacity, _, hits in held)
    assert model._layer_cache.bytes_used == entry_bytes(sum(capacity for _, capacity, _, _ in held), n1, n2, False)
    assert sum(hits for _, _, _, hits in held) == int(uncached(model, *syn.camera(H, W, 15.0), fids(True, L))[4][:, 1:].sum())


@pytest.mark.parametrize("n1,n2", SAMPLES)
@pytest.mark.parametrize("precision,schedule", [("fp32", "stage"), ("fp32", "per_net")])
def test_third_frame_is_bit_identical_fp32(n1, n2, precision, schedule):
    _third_frame_case(n1, n2, precision=precision, schedule=schedule)


@pytest.mark.parametrize("n1,n2", SAMPLES)
@pytest.mark.parametrize("case", ["only_coarse", "width 7", "only_coarse per_net"])
def test_third_frame_is_bit_identical_formats(n1, n2, case):
    if case == "only_coarse":
        _third_frame_case(n1, n2, only_coarse=True)
    elif case == "width 7":
        _third_frame_case(n1, n2, retiming=False)
    else:
        _third_frame_case(n1, n2, precision="fp32", schedule="per_net", only_coarse=True, retiming=False)


@pytest.mark.parametrize("n1,n2", SAMPLES)
def test_third_frame_is_bit_identical_rotated_and_instanced(n1, n2):
    def setup(model):
        copy = model.add_instance(1)
        assert copy == 3
        model.rotation = [None, 0.4, None, (-0.3, [0.2, 0.0, 0.1])]
        model.shift = [None, None, None, [0.35, 0.0, 0.2]]
        model.scale = [1.0, 1.0, 1.1, 0.9]
    _third_frame_case(n1, n2, setup=setup, scene=True)


@pytest.mark.parametrize("n1,n2", SAMPLES)
def test_third_frame_is_bit_identical_ray_and_sample_cull(n1, n2):
    def setup(model):
        model.set_occupancy(stnerf_amd.OccupancyGrids(res=8, samples=True))
    _third_frame_case(n1, n2, setup=setup)


@pytest.mark.parametrize("n1,n2", SAMPLES)
def test_third_frame_is_bit_identical_termination(n1, n2):
    """A cached performer is not terminated: the reference frame has that layer's terminate flag off (the background's stays on)."""
    _third_frame_case(n1, n2, setup=lambda m: m.set_termination(1e-2), reference_setup=lambda m: m.set_termination(1e-2, layers=[]))


@pytest.mark.parametrize("n1,n2", SAMPLES)
def test_third_frame_is_bit_identical_with_a_background_cache(n1, n2):
    model = _third_frame_case(n1, n2, background_cache=True)
    assert model._bkgd_cache.stats == dict(hits=2 * PIECES, misses=PIECES, captures=PIECES, skipped_over_budget=0)


@pytest.mark.parametrize("n1,n2", SAMPLES)
def test_third_frame_is_bit_identical_without_motion_reuse(n1, n2, monkeypatch):
    monkeypatch.setenv("STNERF_MOTION_REUSE", "0")
    _third_frame_case(n1, n2)


# ---- 3. the launch record -------------------------------------------------------------------------------------------------------
NETWORKS = ("mlp_stage", "spacenet", "motionnet")


@pytest.mark.parametrize("precision,schedule", [("bf16x3", "stage"), ("fp32", "per_net")])
def test_reuse_frame_launches_no_network_and_a_nudge_only_its_own(precision, schedule):
    model = make_model(2, 8, 8, precision, schedule, background_cache=True)
    model.scale, model.shift = [1.0, 1.0, 1.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    K, T = syn.camera(H, W, 15.0)
    f = fids(True, 2)
    _, first = render(model, K, T, f, profile=True)
    _, capture = render(model, K, T, f, profile=True)
    third, reuse = render(model, K, T, f, profile=True)
    listed = lambda recs, kind: [r for r in recs if r["kernel"] == "copy_layer_raw_listed" and r["kind"] == kind]
    assert [r for r in first if r["kernel"] in NETWORKS] and not listed(first, 0) and not listed(first, 1)
    assert len(listed(capture, 1)) == 2 * 2 * PIECES and not listed(capture, 0)          # two layers, two stages
    assert not [r for r in reuse if r["kernel"] in NETWORKS], "a frame with every layer cached launched a network kernel"
    assert len(listed(reuse, 0)) == 2 * 2 * PIECES and sorted({r["tag"] for r in listed(reuse, 0)}) == [1, 2]
    assert all(r["bytes_per_ray"] == 32 * r["ns"] + 4 and r["ns"] in (8, 16) for r in listed(reuse, 0) + listed(capture, 1))
    assert_bit_equal(third, uncached(model, K, T, f), "every layer cached")
    # performer 2 nudged: the networks run on performer 2's rows only
    model.shift = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.15, 0.0, 0.05]]
    nudged, recs = render(model, K, T, f, profile=True)
    nets = [r for r in recs if r["kernel"] in NETWORKS]
    assert nets and sorted({r["tag"] for r in listed(recs, 0)}) == [1]
    if schedule == "per_net":
        assert {r["tag"] for r in nets} == {2}, "a network ran on another layer than the nudged one"
        assert len([r for r in nets if r["kernel"] == "spacenet"]) == 2 * PIECES
    else:
        # one stage launch per stage and piece (the stand-alone MotionNet launches are performer 2's: tagged with the layer)
        assert len([r for r in nets if r["kernel"] == "mlp_stage"]) == 2 * PIECES
        assert {r["tag"] for r in nets if r["kernel"] == "motionnet"} <= {2}
    assert_bit_equal(nudged, uncached(model, K, T, f), "performer 2 nudged")
    assert model._layer_cache.stats(mismatch=True)["mismatch"] == 0


# ---- 4. hits and misses of layer 1 ------------------------------------------------------------------------------------------------
def test_layer_1_hits_when_others_change_and_misses_when_it_does():
    model = make_model(2, 8, 8)
    model.scale, model.shift = [1.0, 1.0, 1.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    model.rotation, model.layer_alpha = [None, 0.0, 0.0], [1.0, 1.0, 1.0]
    K, T = syn.camera(H, W, 15.0)
    kw = dict(frame_ids=[1.0, 2.0, 3.0], thr=0.0, bthr=0.0)
    calls = recorded(model._layer_cache)

    def warm():
        for _ in range(3):
            got = render(model, K, T, **kw)
        return got

    def check(what, hit):
        del calls[:]
        got = render(model, K, T, **kw)
        seen = {m for i, m in calls if i == 1}
        assert seen == ({REUSE} if hit else {OFF}), (what, calls)
        assert_bit_equal(got, uncached(model, K, T, **kw), what)

    warm()
    check("nothing changed", True)
    model.shift = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 0.05]]
    check("performer 2's shift", True)
    model.rotation = [None, 0.0, 0.5]
    check("performer 2's rotation", True)
    kw["frame_ids"] = [1.0, 2.0, 1.5]
    check("performer 2's frame id", True)
    model.layer_alpha = [1.0, 0.5, 0.25]
    check("layer_alpha", True)
    kw["bthr"] = 3.0
    check("bkgd_density_threshold", True)
    model.layer_alpha = [1.0, 1.0, 1.0]
    # density_threshold with retiming: the coarse composite zeroes layer 1's densities below it before the resampler reads the
    # layer's weights, so the layer's fine samples move -- a miss.  The threshold must bite IN PART: the median of the positive
    # densities of layer 1's own networks over its box (at its frame id), so that about half of its dense samples go.
    plain = render(model, K, T, **kw)
    sigma = model.density_grid(1, kw["frame_ids"][1], res=8, fine=False)[0]
    assert (sigma > 0).any(), "layer 1 has no density in its box: the case shows nothing"
    kw["thr"] = float(sigma[sigma > 0].median())
    del calls[:]
    cut = render(model, K, T, **kw)
    assert {m for i, m in calls if i == 1} == {OFF}, ("density_threshold under retiming must miss", calls)
    assert_bit_equal(cut, uncached(model, K, T, **kw), "density_threshold, first frame")
    assert not torch.equal(cut[0], plain[0]) and not torch.equal(cut[2][:, 1], plain[2][:, 1]), "the threshold did not change layer 1"
    assert float(cut[2][:, 1, 4].max()) > 0, "the threshold removed layer 1 altogether: it must bite in part"
    warm()
    check("the same threshold again: reused at a threshold that bites", True)
    kw["thr"] = 0.5 * kw["thr"]
    check("another density_threshold", False)
    warm()
    model.hide_layer(2)
    check("hiding layer 2", True)
    model.show_layer(2)
    check("showing it again", True)
    # layer 1's own inputs
    model.shift = [[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.1, 0.0, 0.05]]
    check("its shift", False)
    warm()
    model.scale = [1.0, 1.1, 1.0]
    check("its scale", False)
    warm()
    model.rotation = [None, 0.3, 0.5]
    check("its rotation", False)
    warm()
    kw["frame_ids"] = [1.0, 2.5, 1.5]
    check("its frame id", False)
    warm()
    with torch.no_grad():
        next(model.spacenets[0].parameters()).add_(1e-3)
    check("an in-place update of its SpaceNet", False)
    with torch.no_grad():
        next(model.spacenets[0].parameters()).sub_(1e-3)
    warm()
    grids = stnerf_amd.OccupancyGrids(auto=False)
    model.set_occupancy(grids)
    check("grids attached, none on layer 1", True)
    box = model.layer_box_at(1, 2.5)
    grids.set_manual(1, torch.ones(2, 2, 2, dtype=torch.bool), box.min(0)[0].numpy(), box.max(0)[0].numpy())
    check("its grid", False)
    model.set_occupancy(None)
    warm()
    model.seed = 12
    check("the seed", False)
    assert model._layer_cache.stats(mismatch=True)["mismatch"] == 0


# ---- 5. host policy and plumbing ------------------------------------------------------------------------------------------------
def test_over_budget_frames_render_uncached():
    model = make_model(2, 8, 8)
    model.set_layer_cache(stnerf_amd.LayerCache(max_bytes=entry_bytes(1, 8, 8, False) - 1))
    K, T = syn.camera(H, W, 15.0)
    f = fids(True, 2)
    frames = [render(model, K, T, f) for _ in range(3)]
    st = model._layer_cache.stats()
    assert len(model._layer_cache) == 0 and st["captures"] == 0 and st["hits"] == 0
    assert st["sightings"] == 2 * PIECES and st["skipped_over_budget"] == 2 * 2 * PIECES and st["misses"] == 3 * 2 * PIECES
    ref = uncached(model, K, T, f)
    for k, frame in enumerate(frames):
        assert_bit_equal(frame, ref, f"over budget, frame {k + 1}")


def test_a_rank_share_is_cached_under_its_window():
    model = make_model(2, 8, 8)
    K, T = syn.camera(H, W, 15.0)
    f = fids(True, 2)
    share = lambda rank: parallel.render_view_share(model, K, T, H, W, f, rank, 3, 0.0, 0.0, CHUNK, 1, "cuda", "all")
    pieces = lambda rank: (ops.window_size(H * W, rank * W, W, 3 * W) + (CAP // W * W) - 1) // (CAP // W * W)
    for _ in range(3):
        got = share(1)
    assert model.view_key is None and model.view_frame_ids is None
    st = model._layer_cache.stats()
    assert (st["hits"], st["captures"], st["sightings"]) == (2 * pieces(1),) * 3
    other = share(2)
    st2 = model._layer_cache.stats()
    assert st2["hits"] == st["hits"] and st2["sightings"] == st["sightings"] + 2 * pieces(2), "another rank's window must miss"
    model.set_layer_cache(None)
    assert torch.equal(got.view(torch.int32), share(1).view(torch.int32))
    assert torch.equal(other.view(torch.int32), share(2).view(torch.int32))


def test_render_view_is_cached_and_caller_made_rays_are_not():
    model = make_model(2, 8, 8)
    model.fresh_draws_per_call = True
    K, T = syn.camera(H, W, 15.0)
    f = fids(True, 2)
    flat = lambda out: [t for part in (out[0], out[1], *out[2], *out[3]) for t in part] + list(out[4])
    for _ in range(3):
        got = flat(parallel.render_view(model, K, T, H, W, f, chuncks=CHUNK))
    st = model._layer_cache.stats(mismatch=True)
    assert st["hits"] == 2 * PIECES and st["mismatch"] == 0 and model.seed == 11, "the seed is pinned while the cache is attached"
    with torch.no_grad():
        model(ops.generate_rays(K, T, H, W, frame_ids=f))
    assert model._layer_cache.stats()["hits"] == 2 * PIECES and model.seed == 11
    model.set_layer_cache(None)
    model.fresh_draws_per_call = False
    ref = flat(parallel.render_view(model, K, T, H, W, f, chuncks=CHUNK))
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
    model.fresh_draws_per_call = True
    parallel.render_view(model, K, T, H, W, f, chuncks=CHUNK)
    assert model.seed == 12, "detached: the seed advances again"
    model.fresh_draws_per_call = False


def test_density_threshold_sweep_hits_without_retiming():
    """Width-7 rays apply no threshold (the reference thresholds in retiming mode only): a sweep over it reuses every layer."""
    model = make_model(2, 8, 8)
    K, T = syn.camera(H, W, 15.0)
    f = fids(False, 2)
    for _ in range(3):
        render(model, K, T, f)
    calls = recorded(model._layer_cache)
    got = render(model, K, T, f, thr=5.0, bthr=3.0)
    assert {m for _, m in calls} == {REUSE}
    assert_bit_equal(got, uncached(model, K, T, f, thr=5.0, bthr=3.0), "thresholds, width 7")
