"""The background cache (stnerf_amd.BackgroundCache, stnerf_render_rays_cached): frames of a fixed view evaluate the background
networks once; a frame rendered from the cache must be bit-identical to the frame rendered without one -- all five outputs, every
bit --, must hit when only what acts on other layers or after the networks changed, and must miss when an input of the
background's raw outputs changed.  Shapes: views of 23 x 17 = 391 rays (no multiple of 64 or 128) in launch pieces of 128 (four
pieces, the last one of 7 rays), (n1, n2) = (12, 6) and (8, 0), two performers and none (l == 1: the network stages of a reuse
frame are empty)."""
import types

import pytest
import torch

import stnerf_amd
from stnerf_amd import ops, parallel, synthetic as syn
from stnerf_amd.bkgd_cache import piece_bytes, view_key

pytestmark = pytest.mark.gpu

H, W, CAP, CHUNK = 17, 23, 128, 64
PIECES = (H * W + CAP - 1) // CAP


def build(L, bkgd_space_time=False):
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=bkgd_space_time,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    cfg = types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L))
    model = build_layered_model(cfg, camera_num=1)
    model.load_state_dict(syn.make_state_dict(L, True, True, seed=3, bkgd_use_space_time=bkgd_space_time))
    return model.cuda().eval()


_MODELS = {}


def make_model(L=2, n1=12, n2=6, precision="bf16x3", schedule="stage", bkgd_space_time=False):
    """A model in a known state (the networks are built and uploaded once per flavour) with a fresh cache attached."""
    key = (L, bkgd_space_time)
    if key not in _MODELS:
        _MODELS[key] = build(L, bkgd_space_time)
    model = _MODELS[key]
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.coarse_ray_sample, model.fine_ray_sample = n1, n2
    model.set_precision(precision)
    model.mlp_schedule = schedule
    model.max_rays_per_launch = CAP
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale = model.shift = None
    model.near, model.alpha = 0, 1
    for i in range(L + 1):
        model.show_layer(i)
    model.set_background_cache(stnerf_amd.BackgroundCache())
    return model


def fids(retiming, L, performers=(1.0, 1.0), bkgd=1.0):
    """The frame-id columns of a view: one per layer (retiming, ray width 7 + L) or a single one (width 7)."""
    return [bkgd] + list(performers[:L]) if retiming and L else [float(performers[0])]


def render(model, K, T, frame_ids, h=H, w=W, only_coarse=False, thr=0.0, bthr=0.0, profile=False):
    """The five library outputs of the view, rendered as parallel.render_view_share renders a rank's rays: generated on the device,
    the view key set around the call.  With `profile` also the launch records."""
    rays = ops.generate_rays(K, T, h, w, frame_ids=frame_ids)
    model.view_key = view_key(K, T, h, w, frame_ids) if model._bkgd_cache is not None else None
    try:
        if profile:
            ops.profile_begin()
        with torch.no_grad():
            out = model.render_rays_raw(rays, only_coarse, thr, bthr, ref_chunk=CHUNK)
        torch.cuda.synchronize()
        recs = ops.profile_end() if profile else None
    finally:
        model.view_key = None
    out = [o.clone() for o in out]
    return (out, recs) if profile else out


def uncached(model, *a, **kw):
    cache = model._bkgd_cache
    model.set_background_cache(None)
    try:
        return render(model, *a, **kw)
    finally:
        model.set_background_cache(cache)


def assert_bit_equal(got, ref, what=""):
    assert len(got) == len(ref) == 5
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        av = a.view(torch.uint8) if a.dtype == torch.uint8 else a.contiguous().view(torch.int32)
        bv = b.view(torch.uint8) if b.dtype == torch.uint8 else b.contiguous().view(torch.int32)
        assert torch.equal(av, bv), f"{what}: output {k}: {(av != bv).sum().item()} elements differ"


def stats(model):
    s = model._bkgd_cache.stats
    return s["hits"], s["misses"], s["captures"], s["skipped_over_budget"]


# ---- 1. a hit frame equals the frame rendered without a cache, bit for bit
@pytest.mark.parametrize("L,n1,n2,precision,schedule,only_coarse,retiming", [
    (2, 12, 6, "bf16x3", "stage", False, True),
    (2, 12, 6, "fp32", "stage", False, True),
    (2, 12, 6, "fp32", "per_net", False, True),
    (2, 12, 6, "bf16x3", "stage", True, True),
    (2, 12, 6, "fp32", "per_net", True, False),
    (2, 12, 6, "bf16x3", "stage", False, False),
    (2, 8, 0, "bf16x3", "stage", False, True),
    (2, 8, 0, "fp32", "stage", False, False),
    (0, 12, 6, "bf16x3", "stage", False, False),
    (0, 12, 6, "fp32", "stage", True, False),
    (0, 8, 0, "fp32", "per_net", False, False),
])
def test_hit_frame_is_bit_identical_to_the_uncached_frame(L, n1, n2, precision, schedule, only_coarse, retiming):
    model = make_model(L, n1, n2, precision, schedule)
    K, T = syn.camera(H, W, 15.0)
    fa, fb = fids(retiming, L, (1.0, 1.0)), fids(retiming, L, (2.5, 3.0))
    assert len(fa) == (1 + L if retiming else 1)
    a = render(model, K, T, fa, only_coarse=only_coarse)
    assert stats(model) == (0, PIECES, PIECES, 0)
    assert_bit_equal(a, uncached(model, K, T, fa, only_coarse=only_coarse), "capture frame")
    b = render(model, K, T, fb, only_coarse=only_coarse)
    assert stats(model) == (PIECES, PIECES, PIECES, 0)
    assert_bit_equal(b, uncached(model, K, T, fb, only_coarse=only_coarse), "hit frame")
    if L:
        assert not torch.equal(a[1], b[1]), "the two frames should differ (the performers moved)"
    entry_bytes = sum(t.numel() * 4 for e in model._bkgd_cache._entries.values() for t in e if t is not None)
    assert entry_bytes == model._bkgd_cache.bytes_used == piece_bytes(H * W, n1, n2, only_coarse)


def test_render_view_sets_the_key():
    """parallel.render_view (what render_pose and the renderer's render_path call) is cached; forward() with caller-made rays is not."""
    model = make_model()
    K, T = syn.camera(H, W, 15.0)
    flat = lambda out: [t for part in (out[0], out[1], *out[2], *out[3]) for t in part] + list(out[4])
    a = flat(parallel.render_view(model, K, T, H, W, [1.0, 1.0, 1.0], chuncks=CHUNK))
    b = flat(parallel.render_view(model, K, T, H, W, [1.0, 2.5, 3.0], chuncks=CHUNK))
    assert stats(model) == (PIECES, PIECES, PIECES, 0) and model.view_key is None
    model.set_background_cache(None)
    ref = flat(parallel.render_view(model, K, T, H, W, [1.0, 2.5, 3.0], chuncks=CHUNK))
    assert all(torch.equal(x, y) for x, y in zip(b, ref)) and not torch.equal(a[0], b[0])
    model.set_background_cache(stnerf_amd.BackgroundCache())
    with torch.no_grad():
        model(ops.generate_rays(K, T, H, W, frame_ids=[1.0, 2.5, 3.0]))
    assert stats(model) == (0, 0, 0, 0)


def test_tagged_view_rays_are_cached_through_layered_batchify_ray():
    """The drop-in's device ray generation tags the rays it makes from a camera; the reference's render_pose hands that tensor to
    layered_batchify_ray, which may then serve it from the cache.  A copy, a slice or a tensor written to is never cached."""
    from stnerf_amd.bkgd_cache import tag_view_rays
    from stnerf_amd.utils import layered_batchify_ray
    model = make_model()
    model.fresh_draws_per_call = True                  # (what models built through the patched reference start with)
    K, T = syn.camera(H, W, 15.0)
    flat = lambda out: [t for part in (out[0], out[1], *out[2], *out[3]) for t in part] + list(out[4])

    def frame(f, tag=True, touch=None):
        rays = ops.generate_rays(K, T, H, W, frame_ids=f)
        if tag:
            tag_view_rays(rays, K, T, H, W, f)
        rays = rays.cuda()                             # (as the reference's render_pose does: the same tensor)
        if touch == "write":
            rays[0, 6] += 0.0
        elif touch == "copy":
            rays = rays.clone()
        with torch.no_grad():
            return flat(layered_batchify_ray(model, rays, None, None, chuncks=CHUNK, density_threshold=0.0, bkgd_density_threshold=0.0))

    frame([1.0, 1.0, 1.0])
    b = frame([1.0, 2.5, 3.0])
    assert stats(model) == (PIECES, PIECES, PIECES, 0) and model.seed == 11 and model.view_key is None
    for kw in (dict(tag=False), dict(touch="write"), dict(touch="copy")):
        frame([1.0, 2.5, 3.0], **kw)
        assert stats(model) == (PIECES, PIECES, PIECES, 0), kw
    model.set_background_cache(None)
    model.fresh_draws_per_call = False
    ref = frame([1.0, 2.5, 3.0])
    assert all(torch.equal(x, y) for x, y in zip(b, ref))


# ---- 2. the cached data is what gets composited, and the network is not run
def test_hit_frame_copies_the_cache_in_and_runs_no_background_network():
    model = make_model(2, 12, 6, "fp32", "per_net")
    K, T = syn.camera(H, W, 15.0)
    _, cap = render(model, K, T, [1.0, 1.0, 1.0], profile=True)
    b, hit = render(model, K, T, [1.0, 2.5, 3.0], profile=True)
    bkgd_nets = lambda recs: [r for r in recs if r["kernel"] == "spacenet" and r["tag"] == 0]
    copies = lambda recs: [r for r in recs if r["kernel"] == "copy_layer_raw"]
    assert len(bkgd_nets(cap)) == 2 * PIECES and len(bkgd_nets(hit)) == 0
    assert len([r for r in hit if r["kernel"] == "spacenet"]) == 4 * PIECES          # two performers, two stages
    for recs, to_dense in ((cap, 1), (hit, 0)):
        assert len(copies(recs)) == 2 * PIECES
        assert all(r["kind"] == to_dense and r["tag"] == 0 and r["bytes_per_ray"] == 32 * r["ns"] for r in copies(recs))
        assert sorted({r["ns"] for r in copies(recs)}) == [12, 18]
    # the split-bf16 stage launches: still one per stage and piece (the performers), and the copies
    model = make_model(2, 12, 6, "bf16x3")
    render(model, K, T, [1.0, 1.0, 1.0])
    b, hit = render(model, K, T, [1.0, 2.5, 3.0], profile=True)
    assert len(copies(hit)) == 2 * PIECES and len([r for r in hit if r["kernel"] == "mlp_stage"]) == 2 * PIECES
    # without performers the reuse frame launches no network stage at all
    solo = make_model(0, 12, 6, "bf16x3")
    render(solo, K, T, [1.0])
    _, hit0 = render(solo, K, T, [2.0], profile=True)
    assert len(copies(hit0)) == 2 * PIECES and not [r for r in hit0 if r["kernel"] in ("mlp_stage", "spacenet", "motionnet")]
    # what is in the cache is what is composited
    for entry in model._bkgd_cache._entries.values():
        for t in entry:
            t.fill_(0.25)
    c = render(model, K, T, [1.0, 2.5, 3.0])
    assert stats(model)[0] == 2 * PIECES
    assert not torch.equal(b[0], c[0]), "the mixed image did not change with the cache's contents"


# ---- 3. still a hit when only what acts on other layers, or after the networks, changes
def test_changes_that_do_not_reach_the_background_networks_hit():
    model = make_model()
    # (edits are on from the first frame: switching `scale` on gives layer 0 a scale-1 un-edit through the pivot, which may move
    # its sample points by an ulp -- that is a different background and, rightly, a miss)
    model.scale, model.shift = [1.0, 1.0, 1.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    K, T = syn.camera(H, W, 15.0)
    kw = dict(frame_ids=[1.0, 1.0, 1.0], thr=0.0, bthr=0.0)
    seen, changed = [render(model, K, T, **kw)], []
    assert stats(model) == (0, PIECES, PIECES, 0)

    def check(what):
        got = render(model, K, T, **kw)
        assert stats(model) == (len(seen) * PIECES, PIECES, PIECES, 0), what
        assert_bit_equal(got, uncached(model, K, T, **kw), what)
        # (not every step must show: a synthetic performer network may be empty -- sigma <= 0 in its whole box -- or lie behind the
        # dense background; the steps that did change one of the five outputs are counted at the end)
        if not any(all(torch.equal(a, b) for a, b in zip(got, s)) for s in seen):
            changed.append(what)
        seen.append(got)

    kw["frame_ids"] = [1.0, 2.5, 3.0]
    check("performer frame ids")
    model.hide_layer(1)
    check("hide_layer")
    model.show_layer(1)
    model.hide_layer(2)
    check("show_layer")
    model.show_layer(2)
    model.shift = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.05], [0.0, 0.0, 0.0]]
    check("performer shift")
    model.scale = [1.0, 1.0, 1.2]
    check("performer scale")
    model.alpha = 0.5
    check("alpha")
    kw["thr"] = 5.0
    check("density_threshold")
    kw["bthr"] = 3.0
    check("bkgd_density_threshold")
    assert "performer frame ids" in changed and len(changed) >= 4, f"the sweep barely changed the frames: {changed}"


# ---- 4. a miss when an input of the background's raw outputs changes
def test_changes_that_reach_the_background_networks_miss():
    model = make_model()
    K, T = syn.camera(H, W, 15.0)
    state = dict(K=K, T=T, h=H, w=W)
    f = [1.0, 2.5, 3.0]
    frames = [0]

    def check(what, hit=False, pieces=PIECES):
        before = stats(model)
        got = render(model, state["K"], state["T"], f, h=state["h"], w=state["w"])
        after = stats(model)
        want = (pieces, 0, 0, 0) if hit else (0, pieces, pieces, 0)
        assert tuple(x - y for x, y in zip(after, before)) == want, what
        assert_bit_equal(got, uncached(model, state["K"], state["T"], f, h=state["h"], w=state["w"]), what)

    check("first frame")
    check("the same frame again", hit=True)
    state["T"] = syn.camera(H, W, 16.0)[1]
    check("pose")
    state["K"] = K.clone()
    state["K"][0, 0] *= 1.01
    check("K")
    state["h"] = H - 1
    check("h", pieces=((H - 1) * W + CAP - 1) // CAP)
    state["h"], state["w"] = H, W - 1
    check("w", pieces=(H * (W - 1) + CAP - 1) // CAP)
    state["w"] = W
    check("back to the first size: the view of the 'K' step is still held", hit=True)
    model.seed = 12
    check("seed")
    model.near = 0.5
    check("near")
    model.shift = [[0.1, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    check("layer-0 shift")
    model.set_bkgd_bbox(syn.scene_boxes(2)[0] * 0.9)
    check("background box")
    model.set_precision("fp32")
    check("precision")
    model.mlp_schedule = "per_net"
    check("schedule of the exact-f32 arithmetic")
    with torch.no_grad():
        next(model.bkgd_spacenet.parameters()).add_(1e-3)
    check("in-place update of a bkgd_spacenet parameter")
    with torch.no_grad():
        next(model.bkgd_spacenet.parameters()).sub_(1e-3)
    check("and back (the version moved on)")
    check("nothing changed", hit=True)
    # the background's frame id: an input of its networks with BKGD_USE_SPACE_TIME only
    f = [2.0, 2.5, 3.0]
    check("background frame id, default flags", hit=True)
    model = make_model(bkgd_space_time=True)
    f = [1.0, 2.5, 3.0]
    check("BKGD_USE_SPACE_TIME: first frame")
    f = [1.0, 1.0, 2.0]
    check("BKGD_USE_SPACE_TIME: performer frame ids", hit=True)
    f = [2.0, 1.0, 2.0]
    check("BKGD_USE_SPACE_TIME: background frame id")


# ---- 5. the copy kernel against raw[:, layer], both directions, between canaries
GUARD = 1024                                  # words
PATTERN = 0x7FC00A5A


def guarded(shape):
    numel = 1
    for d in shape:
        numel *= d
    buf = torch.full((numel + 2 * GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + numel].view(torch.float32).reshape(shape)


def intact(buf):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[-GUARD:] == PATTERN).all())


@pytest.mark.parametrize("n", [1, 63, 65, 391])
def test_copy_layer_raw_is_the_layer_slice(n):
    g = torch.Generator().manual_seed(n)
    for ns in (3, 18, 192):
        for l in (1, 3, 9):
            raw_buf, raw = guarded((n, l, ns, 4))
            raw.copy_(torch.randn(n, l, ns, 4, generator=g))
            for layer in range(l):
                dense_buf, dense = guarded((n, ns, 4))
                assert ops.copy_layer_raw(raw, layer, dense, True) is dense
                assert torch.equal(dense.view(torch.int32), raw[:, layer].contiguous().view(torch.int32)), (n, ns, l, layer)
                back_buf, back = guarded((n, l, ns, 4))
                back.copy_(raw)
                fresh = torch.randn(n, ns, 4, generator=g).cuda()
                want = back.clone()
                want[:, layer] = fresh
                assert ops.copy_layer_raw(back, layer, fresh, False) is back
                assert torch.equal(back.view(torch.int32), want.view(torch.int32)), (n, ns, l, layer)   # (the other layers: untouched)
                assert intact(dense_buf) and intact(back_buf) and intact(raw_buf), (n, ns, l, layer)
    with pytest.raises(ValueError, match="bad shape"):
        ops.copy_layer_raw(raw, 9, dense, True)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.copy_layer_raw(raw, 0, torch.empty(n * 192 * 4 + 1, device="cuda")[1:].view(n, 192, 4), True)


# ---- 6. sharding: the ray window is part of the key
def test_a_rank_share_is_cached_under_its_window():
    model = make_model()
    K, T = syn.camera(H, W, 15.0)
    share = lambda rank, f: parallel.render_view_share(model, K, T, H, W, f, rank, 3, 0.0, 0.0, CHUNK, 1, "cuda", "all")
    n_local = ops.window_size(H * W, W, W, 3 * W)
    pieces = (n_local + (CAP // W * W) - 1) // (CAP // W * W)          # launch pieces start on stripe boundaries
    share(1, [1.0, 1.0, 1.0])
    assert stats(model) == (0, pieces, pieces, 0)
    got = share(1, [1.0, 2.5, 3.0])
    assert stats(model) == (pieces, pieces, pieces, 0) and got.shape[0] == n_local
    other = share(2, [1.0, 2.5, 3.0])
    pieces2 = (ops.window_size(H * W, 2 * W, W, 3 * W) + (CAP // W * W) - 1) // (CAP // W * W)
    assert stats(model) == (pieces, pieces + pieces2, pieces + pieces2, 0), "another rank's window must miss"
    model.set_background_cache(None)
    assert torch.equal(got.view(torch.int32), share(1, [1.0, 2.5, 3.0]).view(torch.int32))
    assert torch.equal(other.view(torch.int32), share(2, [1.0, 2.5, 3.0]).view(torch.int32))


# ---- 7. a view that does not fit the budget is rendered without the cache
def test_over_budget_renders_uncached():
    model = make_model()
    model.set_background_cache(stnerf_amd.BackgroundCache(max_bytes=piece_bytes(7, 12, 6, False) - 1))   # smaller than the 7-ray piece
    K, T = syn.camera(H, W, 15.0)
    f = [1.0, 2.5, 3.0]
    got = render(model, K, T, f)
    again = render(model, K, T, f)
    assert stats(model) == (0, 2 * PIECES, 0, 2 * PIECES) and len(model._bkgd_cache) == 0
    ref = uncached(model, K, T, f)
    assert_bit_equal(got, ref, "over budget")
    assert_bit_equal(again, ref, "over budget, again")
    # room for the last piece only: it is cached, the others are not
    model.set_background_cache(stnerf_amd.BackgroundCache(max_bytes=piece_bytes(7, 12, 6, False)))
    render(model, K, T, f)
    assert_bit_equal(render(model, K, T, f), ref, "partly cached")
    assert stats(model) == (1, 2 * PIECES - 1, 1, 2 * (PIECES - 1))


# ---- 8. a cached run keeps one jitter pattern
def test_seed_is_pinned_while_a_cache_is_attached():
    model = make_model()
    model.fresh_draws_per_call = True
    K, T = syn.camera(H, W, 15.0)
    render(model, K, T, [1.0, 1.0, 1.0])
    b = render(model, K, T, [1.0, 2.5, 3.0])
    assert model.seed == 11 and stats(model) == (PIECES, PIECES, PIECES, 0)
    model.set_background_cache(None)
    ref = render(model, K, T, [1.0, 2.5, 3.0])
    assert model.seed == 12, "detached: the seed advances again"
    assert_bit_equal(b, ref, "seed 11")
