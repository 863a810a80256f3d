"""The layer cache's host side (no GPU): the key of a layer's launch piece (LayeredRFRender.layer_cache_key) holds exactly the inputs
of that layer's raw network outputs and nothing of the other layers; LayerCache's three-sighting policy, budget and eviction with a
stub in place of the device tensors; the numpy restatement of the listed copy against a plain loop; the argument errors of the two
new entries, refused before any launch; the exports and the ctypes mirror of stnerf_layer_cache."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

import stnerf_amd
from conftest import REPO
from layer_cache_common import check_listed_copy_argument_errors, listed_copy_loop, listed_copy_reference, ray_lists
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.bkgd_cache import tag_view_rays, tagged_view_frame_ids, view_frame_ids, view_key
from stnerf_amd.layer_cache import CAPTURE, OFF, REUSE, LayerCache, dense_bytes, entry_bytes


def make_model(L=2):
    """A model on the HOST: the key is host arithmetic and never touches the weights' values."""
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    model = build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L)), camera_num=1)
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.seed = 11
    model.scale, model.shift = [1.0] * (L + 1), [[0.0, 0.0, 0.0] for _ in range(L + 1)]
    model.rotation = [None] + [0.0] * L
    return model.eval()


def key_of(model, i=1, K=None, T=None, h=17, w=23, frame_ids=(1.0, 2.0, 3.0), piece=(0, 128), window=(0, 0, 0), retiming=True,
           only_coarse=False, thr=1e-4):
    K0, T0 = syn.camera(17, 23, 15.0)
    return model.layer_cache_key(i, view_key(K0 if K is None else K, T0 if T is None else T, h, w, list(frame_ids)), piece, window,
                                 retiming, only_coarse, frame_ids=view_frame_ids(frame_ids), density_threshold=thr)


# ---- the key ----------------------------------------------------------------------------------------------------------------
def test_key_ignores_the_other_layers_and_what_acts_after_the_networks():
    model = make_model()
    base = key_of(model)
    assert base == key_of(model) and hash(base) == hash(key_of(model))
    assert key_of(model, 2) != base and key_of(model, 2)[1] == base[1], "the layer belongs to the group"
    assert key_of(model, frame_ids=(5.0, 2.0, 1.5)) == base                        # the background's and performer 2's frame ids
    model.shift = [[0.3, 0.0, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 0.05]]             # their shifts, scales and rotations
    model.scale = [1.3, 1.0, 1.2]
    model.rotation = [0.2, 0.0, (0.5, [0.0, 0.1, 0.0])]
    assert key_of(model) == base
    model.hide_layer(2)                                                            # display_layers: the others' and its own
    model.hide_layer(1)
    assert key_of(model) == base
    model.show_layer(1)
    model.show_layer(2)
    model.alpha = 0.5                                                              # opacities
    assert key_of(model) == base
    model.alpha, model.layer_alpha = 1.0, [1.0, 0.25, 0.5]
    assert key_of(model) == base
    model.set_termination(1e-3)                                                    # the termination settings
    assert key_of(model) == base
    model.set_termination(None)
    with torch.no_grad():                                                          # the other networks
        next(model.spacenets[1].parameters()).add_(1e-3)
        next(model.bkgd_spacenet.parameters()).add_(1e-3)
    assert key_of(model) == base
    model.set_bkgd_bbox(model.bkgd_bbox * 0.9)                                     # (the pivot reads bkgd_bbox's centre row 0 only ...
    per = model.bboxes.clone()
    per[1:, 1] += 0.25                                                             # ... and frame 0 of the table: later frames of performer 2 move)
    model.set_bboxes(per)
    assert key_of(model) == base
    grids = stnerf_amd.OccupancyGrids(auto=False)                                  # grids attached, none on this layer
    model.set_occupancy(grids)
    assert key_of(model) == base
    grids.set_manual(2, torch.ones(2, 2, 2, dtype=torch.bool), [0, 0, 0], [1, 1, 1])
    assert key_of(model) == base and key_of(model, 2) != key_of(make_model(), 2)
    # bkgd_density_threshold is no argument of the key; density_threshold is one, and counts only where it reaches the layer's fine
    # samples: with retiming (width-7 rays apply no threshold) and a fine stage
    assert key_of(model, frame_ids=(2.0,), retiming=False, thr=5.0) == key_of(model, frame_ids=(2.0,), retiming=False, thr=None)
    assert key_of(model, only_coarse=True, thr=5.0) == key_of(model, only_coarse=True, thr=None)
    # an instance of another performer changes the ray width, a different format; one of THIS performer is a layer of its own
    wide = make_model()
    assert wide.add_instance(2) == 3
    wide.scale, wide.shift, wide.rotation = [1.0] * 4, [[0.0, 0.0, 0.0] for _ in range(4)], [None, 0.0, 0.0, None]
    assert key_of(wide, frame_ids=(1.0, 2.0, 3.0, 3.0))[0][:10] == base[0][:10]


def test_key_changes_with_every_input_of_the_layer():
    model = make_model()
    base = key_of(model)
    K, T = syn.camera(17, 23, 15.0)
    seen = {base}

    def differs(key, what):
        assert key not in seen, what
        seen.add(key)

    differs(key_of(model, T=syn.camera(17, 23, 16.0)[1]), "pose")
    K2 = K.clone()
    K2[0, 0] *= 1.01
    differs(key_of(model, K=K2), "K")
    differs(key_of(model, h=16), "h")
    differs(key_of(model, w=22), "w")
    differs(key_of(model, piece=(128, 256), window=(128, 0, 0)), "piece")
    differs(key_of(model, window=(23, 23, 69)), "ray window")
    assert key_of(model, window=(23, 23, 69))[0] == base[0], "the window belongs to the piece part"
    differs(key_of(model, only_coarse=True), "only_coarse")
    differs(key_of(model, thr=5.0), "density_threshold under retiming: the coarse composite applies it before the resampler")
    differs(key_of(model, thr=0.0), "density_threshold 0")
    with pytest.raises(ValueError, match="density_threshold"):
        key_of(model, thr=None)
    differs(key_of(model, frame_ids=(1.0, 2.5, 3.0)), "its frame id")
    differs(key_of(model, frame_ids=(2.0,), retiming=False), "ray format (width 7: the one frame id is the layer's)")
    differs(key_of(model, frame_ids=(3.0,), retiming=False), "width 7, another frame id")
    for attr, value, what in (("seed", 12, "seed"), ("near", 0.5, "near"), ("boarder_weight", 1e9, "border"),
                              ("coarse_ray_sample", 8, "n1"), ("fine_ray_sample", 0, "n2")):
        old = getattr(model, attr)
        setattr(model, attr, value)
        differs(key_of(model), what)
        setattr(model, attr, old)
        assert key_of(model) == base, what
    model.shift = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.0]]
    differs(key_of(model), "its shift")
    model.shift = [[0.0, 0.0, 0.0], None, [0.0, 0.0, 0.0]]                        # (fine: no un-edit at all for the layer)
    differs(key_of(model), "its shift None")
    model.shift = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    model.scale = [1.0, 1.1, 1.0]
    differs(key_of(model), "its scale")
    model.scale = None
    differs(key_of(model), "no scale edit (no pivot, no scale-1 un-edit)")
    model.scale = [1.0, 1.0, 1.0]
    assert key_of(model) == base
    model.rotation = [None, 0.3, 0.0]
    differs(key_of(model), "its rotation")
    model.rotation = [None, (0.3, [0.1, 0.0, 0.0]), 0.0]
    differs(key_of(model), "its rotation's centre")
    model.rotation = [None, None, 0.0]
    differs(key_of(model), "no rotation")
    model.rotation = [None, 0.0, 0.0]
    assert key_of(model) == base
    per = model.bboxes
    model.set_bboxes(per * torch.tensor([1.0, 1.0, 1.0]))
    assert key_of(model) == base, "a new tensor with the same boxes"
    moved = per.clone()
    moved[1, 0] += 0.25                                                            # (frame 2 of performer 1: its box at frame id 2)
    model.set_bboxes(moved)
    differs(key_of(model), "its box at its frame id")
    model.set_bboxes(per)
    assert key_of(model) == base
    pristine = per.clone()
    per[1, 0] += 0.5                                                               # (in place: the host copy follows the version)
    differs(key_of(model), "its box, in place")
    per.copy_(pristine)
    assert key_of(model) == base
    model.set_precision("fp32")
    differs(key_of(model), "precision")
    model.mlp_schedule = "per_net"
    differs(key_of(model), "schedule of the exact-f32 arithmetic")
    model.mlp_schedule = "stage"
    model.set_precision("bf16x3")
    model.mlp_schedule = "per_net"
    assert key_of(model) == base, "split bf16 has one schedule"
    model.mlp_schedule = "stage"
    for nets, what in ((model.spacenets, "spacenets"), (model.spacenets_fine, "spacenets_fine"), (model.time_deform_nets, "time_deform_nets")):
        with torch.no_grad():
            next(nets[0].parameters()).add_(0.0)                                   # (the version moves on)
        differs(key_of(model), what)
    now = key_of(model)
    grids = stnerf_amd.OccupancyGrids(res=8)
    model.set_occupancy(grids)
    differs(key_of(model), "a built grid")
    grids.dilate = 1
    differs(key_of(model), "its dilation")
    grids.samples = True
    differs(key_of(model), "the sample flag")
    grids.set_manual(1, torch.ones(2, 2, 2, dtype=torch.bool), [0, 0, 0], [1, 1, 1])
    differs(key_of(model), "a manual grid")
    grids.set_manual(1, torch.ones(2, 2, 2, dtype=torch.bool), [0, 0, 0], [1, 1, 2])
    differs(key_of(model), "its bounds")
    model.set_occupancy(None)
    assert key_of(model) == now
    # an instance keys like a layer of its own: its source's networks, its own index, frame id and edits
    copy = model.add_instance(1)
    model.scale, model.shift, model.rotation = [1.0] * 4, [[0.0, 0.0, 0.0] for _ in range(4)], [None, 0.0, 0.0, 0.0]
    a = key_of(model, copy, frame_ids=(1.0, 2.0, 3.0, 2.0))
    b = key_of(model, 1, frame_ids=(1.0, 2.0, 3.0, 2.0))
    assert a != b and a[0][19] == b[0][19], "the same parameter versions, another layer"
    differs(key_of(model, copy, frame_ids=(1.0, 2.0, 3.0, 1.5)), "the instance's frame id")
    with pytest.raises(ValueError, match="not a performer"):
        key_of(model, 0)
    with pytest.raises(ValueError, match="host values"):
        key_of(model, 1, frame_ids=(1.0, 2.0, 3.0))


def test_the_view_frame_ids_travel_with_the_view_key():
    assert view_frame_ids([1, 2.5]) == (1.0, 2.5) and view_frame_ids(None) is None and view_frame_ids([]) is None
    K, T = syn.camera(4, 5, 0.0)
    rays = torch.zeros(20, 9)
    tag_view_rays(rays, K, T, 4, 5, [1.0, 2.5, 3.0])
    assert tagged_view_frame_ids(rays) == (1.0, 2.5, 3.0)
    rays[0, 0] = 1.0
    assert tagged_view_frame_ids(rays) is None, "a tensor written to since carries no tag"
    # render_view_share sets and restores both around the call, with either cache attached
    from stnerf_amd import parallel
    model = make_model()
    assert parallel._view_key(model, K, T, 4, 5, [1.0, 2.0, 3.0]) is None and parallel._view_frame_ids(model, [1.0]) is None
    model.set_layer_cache(LayerCache(max_bytes=0))
    assert parallel._view_key(model, K, T, 4, 5, [1.0, 2.0, 3.0]) == view_key(K, T, 4, 5, [1.0, 2.0, 3.0])
    assert parallel._view_frame_ids(model, [1.0, 2.0, 3.0]) == (1.0, 2.0, 3.0)


def test_seed_is_pinned_while_a_layer_cache_is_attached():
    model = make_model()
    model.fresh_draws_per_call = True
    model.advance_seed()
    assert model.seed == 12
    model.set_layer_cache(LayerCache())
    model.advance_seed()
    assert model.seed == 12
    model.set_layer_cache(None)
    model.advance_seed()
    assert model.seed == 13


# ---- the policy and the budget, a stub in place of the device tensors -------------------------------------------------------------
class Scalar:
    """Stands for a device scalar: counts how often it is read."""
    def __init__(self, value):
        self.value, self.reads = value, 0

    def reshape(self, *_):
        return [self]

    def __int__(self):
        self.reads += 1
        return self.value


def stub_allocate(captured):
    """An ``allocate`` that makes no tensor; the entry's count reads as ``captured[0]`` (what the capture frame would write)."""
    def allocate(capacity, n1, n2, only_coarse, device):
        return "raw_c", None if only_coarse else "raw_f", "rays", Scalar(captured[0])
    return allocate


def frame(cache, key, hits, n1=12, n2=6, only_coarse=False):
    """What LayeredRFRender._render_launch does with one layer of one piece -> the mode of the frame."""
    mode, entry = cache.plan(key, n1, n2, only_coarse, "cpu")
    if entry is None and cache.wants_count(key):
        cache.sighted(key, hits)
    return mode, entry


def test_three_sightings_capture_once_and_then_reuse():
    captured = [40]
    cache = LayerCache(max_bytes=1 << 20, allocate=stub_allocate(captured))
    key = (("layer", 1, "view"), (0, 128, (0, 0, 0)))
    count = Scalar(40)
    assert frame(cache, key, count) == (OFF, None) and count.reads == 0, "the first sighting reads nothing"
    mode, entry = frame(cache, key, Scalar(40))
    assert mode == CAPTURE and entry.capacity == 40 and count.reads == 1, "the second sighting reads the count once"
    assert entry.arg(mode) == ("raw_c", "raw_f", "rays", entry.count, CAPTURE)
    assert cache.bytes_used == entry_bytes(40, 12, 6, False) == 40 * (16 * 30 + 4) and dense_bytes(128, 12, 6, False) == 128 * 16 * 30
    for k in range(3):
        mode, again = frame(cache, key, Scalar(40))
        assert mode == REUSE and again is entry and entry.count.reads == 1, "the captured count is read once, before the first reuse"
    assert entry.hits == 40 and count.reads == 1
    assert cache.stats() == dict(hits=3, misses=2, sightings=1, captures=1, skipped_over_budget=0)
    assert cache.held() == [(key, 40, entry_bytes(40, 12, 6, False), 40)]
    # a layer without a hit ray still gets an entry (one slot)
    empty = (("layer", 2, "view"), (0, 128, (0, 0, 0)))
    captured[0] = 0
    frame(cache, empty, Scalar(0))
    assert frame(cache, empty, Scalar(0))[1].capacity == 1 and frame(cache, empty, Scalar(0))[0] == REUSE
    # only_coarse: no fine slice
    oc = (("layer", 1, "view", "only_coarse"), (0, 128, (0, 0, 0)))
    frame(cache, oc, Scalar(7), only_coarse=True)
    captured[0] = 7
    mode, e = frame(cache, oc, Scalar(7), only_coarse=True)
    assert mode == CAPTURE and e.raw_f is None and e.nbytes == 7 * (16 * 12 + 4)


def test_a_capture_that_did_not_fit_is_discarded():
    captured = [-1]
    cache = LayerCache(max_bytes=1 << 20, allocate=stub_allocate(captured))
    key = (("g",), (0, 8, (0, 0, 0)))
    frame(cache, key, Scalar(5))
    assert frame(cache, key, Scalar(5))[0] == CAPTURE
    assert frame(cache, key, Scalar(5)) == (OFF, None) and len(cache) == 0 and cache.bytes_used == 0, "count == -1: the entry is dropped"
    assert cache.stats()["hits"] == 0 and cache.stats()["sightings"] == 2, "and the key starts over"


def test_a_layer_that_moves_every_frame_never_captures():
    cache = LayerCache(max_bytes=1 << 20, allocate=stub_allocate([9]))
    for t in range(50):
        assert frame(cache, (("layer", 1, t), (0, 8, (0, 0, 0))), Scalar(9)) == (OFF, None)
    assert cache.stats() == dict(hits=0, misses=50, sightings=50, captures=0, skipped_over_budget=0) and len(cache) == 0


def test_budget_evicts_other_groups_oldest_first_and_never_raises(monkeypatch):
    one = entry_bytes(10, 12, 6, False)
    cache = LayerCache(max_bytes=2 * one, allocate=stub_allocate([10]))
    key = lambda g, p=0: ((g,), (p, p + 8, (0, 0, 0)))

    def capture(k):
        frame(cache, k, Scalar(10))
        return frame(cache, k, Scalar(10))[0]

    assert capture(key("a")) == CAPTURE and capture(key("b")) == CAPTURE and cache.bytes_used == 2 * one
    assert frame(cache, key("a"), Scalar(10))[0] == REUSE                       # ("a" is now the most recently used)
    assert capture(key("c")) == CAPTURE and [k[0][0] for k, *_ in cache.held()] == ["a", "c"], "the oldest other group went"
    # the same group is never evicted for its own pieces: the third piece of "c" does not fit and renders uncached
    assert capture(key("c", 8)) == CAPTURE and [k[0][0] for k, *_ in cache.held()] == ["c", "c"]
    assert capture(key("c", 16)) == OFF and cache.stats()["skipped_over_budget"] == 1
    assert frame(cache, key("c", 16), Scalar(10)) == (OFF, None) and cache.stats()["skipped_over_budget"] == 2, "tried again, no new sighting"
    assert cache.stats()["sightings"] == 5 and cache.bytes_used == 2 * one
    # an entry that would not fit even with every other group gone evicts nothing, however often it is tried
    mixed = LayerCache(max_bytes=2 * one, allocate=stub_allocate([10]))
    for g in ("a", "b"):
        frame(mixed, key(g), Scalar(10))
        assert frame(mixed, key(g), Scalar(10))[0] == CAPTURE
    frame(mixed, key("big"), Scalar(30))
    for tries in (1, 2, 3):
        assert frame(mixed, key("big"), Scalar(30)) == (OFF, None)
        assert [k[0][0] for k, *_ in mixed.held()] == ["a", "b"] and mixed.stats()["skipped_over_budget"] == tries
    assert frame(mixed, key("a"), Scalar(10))[0] == REUSE and frame(mixed, key("b"), Scalar(10))[0] == REUSE
    # nothing fits a budget of zero; nothing raises
    none = LayerCache(max_bytes=0, allocate=stub_allocate([10]))
    assert frame(none, key("z"), Scalar(3)) == (OFF, None)
    assert frame(none, key("z"), Scalar(3)) == (OFF, None) and none.stats()["skipped_over_budget"] == 1 and len(none) == 0
    monkeypatch.setenv("STNERF_LAYER_CACHE_GB", "0.5")
    assert LayerCache().max_bytes == 1 << 29
    monkeypatch.delenv("STNERF_LAYER_CACHE_GB")
    assert LayerCache().max_bytes == 8 << 30
    cache.clear()
    assert len(cache) == 0 and cache.bytes_used == 0 and cache.stats()["captures"] == 4


# ---- the listed copy: the numpy restatement against a plain loop ------------------------------------------------------------------
@pytest.mark.parametrize("n,l,ns", [(1, 2, 3), (17, 4, 5), (40, 2, 7)])
def test_numpy_restatement_is_the_plain_loop(n, l, ns):
    rs = np.random.RandomState(n)
    for layer in sorted({1, l - 1}):
        for name, lst in ray_lists(n, rs):
            c = len(lst)
            padded = np.concatenate([lst, np.full(n - c, -7, np.int32)])
            for capacity in sorted({c, c + 3, c - 1} - {-1}):
                raw = rs.standard_normal((n, l, ns, 4)).astype(np.float32)
                dense = rs.standard_normal((capacity, ns, 4)).astype(np.float32)
                rays = np.full(capacity, 77, np.int32)
                a = listed_copy_reference(raw, layer, dense, rays, 12345, True, padded, c)
                b = listed_copy_loop(raw, layer, dense, rays, 12345, True, padded, c)
                assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:] == ((c if c <= capacity else -1), 0)
                if c > capacity:
                    assert np.array_equal(a[1], dense) and np.array_equal(a[2], rays), "nothing but the count is written"
                back = rs.standard_normal((n, l, ns, 4)).astype(np.float32)
                for frame_count in (None, c, c + 1):
                    ra = listed_copy_reference(back, layer, a[1], a[2], a[3], False, None, frame_count, 5)
                    rb = listed_copy_loop(back, layer, a[1], a[2], a[3], False, None, frame_count, 5)
                    assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3])) and ra[3:] == rb[3:]
                    assert ra[4] == 5 + (frame_count is not None and frame_count != a[3])
                    if 0 < c <= capacity:
                        outside = np.ones((n, l), bool)
                        outside[lst, layer] = False
                        assert np.array_equal(ra[0][outside], back[outside]) and np.array_equal(ra[0][lst, layer], raw[lst, layer])
                    else:
                        assert np.array_equal(ra[0], back)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_listed_copy_refuses_bad_arguments_before_any_launch():
    assert check_listed_copy_argument_errors() >= 12


def test_render_rays_layers_checks_its_table_on_the_host():
    lib = hip.lib()
    fake = 1 << 20
    null = C.c_void_p(0)
    p = hip.RenderParams()
    p.l, p.n1, p.n2, p.ray_stride, p.retiming, p.precision = 3, 8, 8, 9, 1, 3
    for i in range(3):
        p.shown[i] = 1
    nets = hip.Nets()
    nets.bkgd = nets.bkgd_fine = fake
    for i in (1, 2):
        nets.space[i] = nets.space_fine[i] = fake

    def call(table, mismatch=null, n=4, only_coarse=0):
        p.only_coarse = only_coarse
        ws = lib.stnerf_render_workspace_bytes(n, 3, 8, 8, only_coarse)
        return lib.stnerf_render_rays_layers(fake, n, fake, 0, C.byref(nets), C.byref(p), null, null, fake, ws, fake, fake, fake, fake, fake,
                                             None, None, null, None, None, null, None, null, 0.0, None, null, None, null, table, mismatch, None)

    def table(**kw):
        t = (hip.LayerCache * 3)()
        t[1] = hip.LayerCache(fake, fake, fake, fake, 4, hip.LAYER_CACHE_REUSE)
        for name, value in kw.items():
            setattr(t[1], name, value)
        return t

    bad = [(table(mode=7), "unknown layer cache mode"), (table(raw_coarse=None), "without raw_coarse"), (table(rays=None), "without raw_coarse"),
           (table(count=None), "without raw_coarse"), (table(raw_fine=None), "without raw_fine"), (table(raw_coarse=fake + 4), "16-byte aligned"),
           (table(raw_fine=fake + 8), "16-byte aligned"), (table(capacity=-1), "negative capacity")]
    for t, message in bad:
        assert call(t) == hip.EINVAL and message in hip.last_error(), (message, hip.last_error())
    zero = table()
    zero[0] = hip.LayerCache(fake, fake, fake, fake, 4, hip.LAYER_CACHE_CAPTURE)
    assert call(zero) == hip.EINVAL and "entry 0 must be OFF" in hip.last_error()
    assert call(table(), mismatch=fake + 4) == hip.EINVAL and "8-byte aligned" in hip.last_error()
    # n == 0: every check passes and nothing is launched; a hidden layer's entry is ignored; only_coarse takes raw_fine == NULL
    assert call(table(), n=0) == hip.OK and call(table(raw_fine=None), n=0, only_coarse=1) == hip.OK
    p.shown[1] = 0
    assert call(table(raw_coarse=None), n=0) == hip.OK
    p.shown[1] = 1


def test_exports_and_struct_layout(tmp_path):
    assert {"stnerf_copy_layer_raw_listed", "stnerf_render_rays_layers"} <= set(hip.exported_symbols())
    assert ops.PROFILE_KERNELS[13] == "copy_layer_raw_listed" and ops.PROFILE_KERNELS[6] == "copy_layer_raw"
    assert (hip.LAYER_CACHE_OFF, hip.LAYER_CACHE_CAPTURE, hip.LAYER_CACHE_REUSE) == (OFF, CAPTURE, REUSE) == (0, 1, 2)
    assert stnerf_amd.LayerCache is LayerCache
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(stnerf_layer_cache));']
    for name, _ in hip.LayerCache._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(stnerf_layer_cache, {name}));')
    lines.append('printf("modes %d %d %d\\n", STNERF_LAYER_CACHE_OFF, STNERF_LAYER_CACHE_CAPTURE, STNERF_LAYER_CACHE_REUSE);')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split(None, 1) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(hip.LayerCache) == 48
    for name, _ in hip.LayerCache._fields_:
        assert int(got[name]) == getattr(hip.LayerCache, name).offset, name
    assert got["modes"].split() == ["0", "1", "2"]
