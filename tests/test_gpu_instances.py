"""Layer instances and per-layer opacity on the GPU.  The definition: a model M with L performers and K
instances renders what its WIDE model W(M) renders -- LAYER_NUM = L + K, the sources' modules and box columns copied -- bit for
bit, through every inference entry.  So every check here is ``torch.equal`` on bit patterns and there is no tolerance.  Shapes as
tests/test_gpu_rotation.py: views of 23 x 17 = 391 rays (no multiple of 64) in launch pieces of 128 (the last one of 7 rays),
reference chunks of 64, (n1, n2) = (12, 6) and (8, 0), a synthetic model with L = 2 (and one with L = 1 for the pivot)."""
import pytest
import torch

import stnerf_amd
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.bkgd_cache import view_key

from instances_common import CASES, base_model, frame_ids, instance_edits, sync_settings, wide_model

pytestmark = pytest.mark.gpu

H, W, CAP, CHUNK = 17, 23, 128, 64
N = H * W
PIECES = (N + CAP - 1) // CAP
NAMES = ("mixed_fine", "mixed_coarse", "layer_fine", "layer_coarse", "mask")

_BASE, _WIDE = {}, {}


def make_model(case="A", n1=12, n2=6, precision="bf16x3", schedule="stage"):
    """The instanced model M of a case in a known state (built and uploaded once per L), without edits."""
    L, sources = CASES[case]
    if L not in _BASE:
        _BASE[L] = base_model(L).cuda()
    model = _BASE[L]
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.clear_instances()
    model.train(False)
    for src in sources:
        model.add_instance(src)
    model.coarse_ray_sample, model.fine_ray_sample = n1, n2
    model.set_precision(precision)
    model.mlp_schedule = schedule
    model.max_rays_per_launch = CAP
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale = model.shift = model.rotation = model.layer_alpha = None
    model.near, model.alpha = 0, 1
    for i in range(model.total_layers):
        model.show_layer(i)
    model.set_background_cache(None)
    return model


def wide_of(model, case):
    """W(M) with M's present settings (the networks built and uploaded once per case)."""
    if case not in _WIDE:
        _WIDE[case] = wide_model(model)
    w = sync_settings(model, _WIDE[case])
    w.set_background_cache(None)
    return w


def edited(model):
    L = model.layer_num
    model.scale, model.shift, model.rotation = instance_edits(model.total_layers, L + 1)
    return model


def view_rays(model, retiming=True, orbit=15.0, frames=None):
    K, T = syn.camera(H, W, orbit)
    f = frames or frame_ids(model.layer_num, len(model.instances))
    return ops.generate_rays(K, T, H, W, frame_ids=list(f) if retiming else [2.0])


def render(model, rays, only_coarse=False):
    with torch.no_grad():
        out = model.render_rays_raw(rays, only_coarse, 0.0, 0.0, ref_chunk=CHUNK)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype in (torch.uint8, torch.bool) else t.contiguous().view(torch.int32)


def assert_bit_equal(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    a, b = bits(got), bits(ref)
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ"


def assert_same_render(got, ref, what=""):
    assert len(got) == len(ref) == 5
    for k, name in enumerate(NAMES):
        assert_bit_equal(got[k], ref[k], f"{what} {name}")


# ---- 1. instanced == wide
GRID = [("bf16x3", "stage", True, False, 12, 6), ("bf16x3", "stage", True, True, 12, 6), ("bf16x3", "stage", False, False, 12, 6),
        ("bf16x3", "stage", False, True, 12, 6), ("fp32", "stage", True, False, 12, 6), ("fp32", "per_net", True, False, 12, 6),
        ("bf16x3", "stage", True, False, 8, 0)]


@pytest.mark.parametrize("precision,schedule,retiming,only_coarse,n1,n2", GRID)
@pytest.mark.parametrize("case", ["A", "B"])
def test_instanced_model_equals_the_wide_model(case, precision, schedule, retiming, only_coarse, n1, n2):
    model = edited(make_model(case, n1, n2, precision, schedule))
    L, l = model.layer_num, model.total_layers
    assert L == 2 and l == 3 + len(CASES[case][1]) and model.instances == CASES[case][1]
    rays = view_rays(model, retiming)
    assert rays.shape == (N, 6 + l if retiming else 7)
    if retiming:                                     # every instance's frame id differs from its source's
        assert all(float(rays[0, 6 + L + 1 + j]) != float(rays[0, 6 + s]) for j, s in enumerate(model.instances))
    before = {m: m._packed(precision).blob.data_ptr() for m in list(model.spacenets) + list(model.time_deform_nets)}
    got = render(model, rays, only_coarse)
    assert got[2].shape == (N, l, 5) and got[4].shape == (N, l)
    assert all(m._packed(precision).blob.data_ptr() == p for m, p in before.items()), "an instance repacked a network"
    ref = render(wide_of(model, case), rays, only_coarse)
    assert_same_render(got, ref, case)
    for j, s in enumerate(model.instances):          # the copies are on the picture, and are no bitwise copy of their source
        i = L + 1 + j
        assert int((got[4][:, i] != 0).sum()) >= 0.05 * N, (i, int((got[4][:, i] != 0).sum()))
        assert bool((got[3][:, i, 4] > 0).any()) and bool((got[3][:, s, 4] > 0).any()), "an empty layer shows nothing"
        assert not torch.equal(got[3][:, i], got[3][:, s])


def test_one_performer_one_instance_takes_its_pivot_from_the_expanded_table():
    """L = 1: the edit pivot is "layers 1 and 2 of the box table", and layer 2 exists only as the instance's column."""
    model = edited(make_model("L1"))
    assert model.layer_num == 1 and model.total_layers == 3
    rays = view_rays(model, True)
    got = render(model, rays)
    wide = wide_of(model, "L1")
    assert torch.equal(model._pivot(), wide._pivot())
    assert_same_render(got, render(wide, rays), "L = 1, K = 1")
    assert int((got[4][:, 2] != 0).sum()) >= 0.05 * N


def test_hidden_instance_equals_the_wide_model_with_that_layer_hidden():
    model = edited(make_model("B"))
    rays = view_rays(model, True)
    shown = render(model, rays)
    model.hide_layer(3)
    assert not model.is_shown_layer(3) and model.is_shown_layer(4)
    got = render(model, rays)
    wide = wide_of(model, "B")
    assert not wide.is_shown_layer(3)
    assert_same_render(got, render(wide, rays), "instance 3 hidden")
    assert not torch.equal(got[0], shown[0])
    model.show_layer(3)
    assert_same_render(render(model, rays), shown, "shown again")


# ---- 2. the scene passes and render_pose
def test_scene_passes_and_render_pose_equal_the_wide_model():
    from stnerf_amd.render.render_pose import render_pose
    model = edited(make_model("B"))
    l = model.total_layers
    rays = view_rays(model, True)
    wide = wide_of(model, "B")
    with torch.no_grad():
        out, scene = model.render_rays_scene(rays, False, 0.0, 0.0, ref_chunk=CHUNK)
        out_w, scene_w = wide.render_rays_scene(rays, False, 0.0, 0.0, ref_chunk=CHUNK)
    assert len(scene) == l and len(out[2]) == l and len(out[3]) == l and len(out[4]) == l
    for i in range(l):
        for a, b, name in zip(scene[i], scene_w[i], ("colour", "depth", "alpha")):
            assert_bit_equal(a, b, f"scene {name} of layer {i}")
        for k in (2, 3):
            for a, b in zip(out[k][i], out_w[k][i]):
                assert_bit_equal(a, b, f"layer output {k} of layer {i}")
        assert_bit_equal(out[4][i], out_w[4][i], f"mask of layer {i}")
    for a, b in zip(out[0] + out[1], out_w[0] + out_w[1]):
        assert_bit_equal(a, b, "mixed")
    K, T = syn.camera(H, W, 15.0)
    pairs = list(enumerate(frame_ids(2, 2)))
    got = render_pose(model, T, K, H, W, pairs, 20.0, 0, 0, scene_passes=True)
    ref = render_pose(wide, T, K, H, W, pairs, 20.0, 0, 0, scene_passes=True)
    assert len(got[2]) == len(got[3]) == l and all(len(v) == l for v in got[4].values())
    assert_bit_equal(got[0], ref[0], "render_pose colour")
    assert_bit_equal(got[1], ref[1], "render_pose depth")
    for a, b in zip(got[2] + got[3], ref[2] + ref[3]):
        assert_bit_equal(a, b, "render_pose layers")
    for key in got[4]:
        for a, b in zip(got[4][key], ref[4][key]):
            assert_bit_equal(a, b, key)


# ---- 3. the background cache: a sweep over an instance's frame id and shift hits
def test_background_cache_hits_while_an_instance_moves():
    model = edited(make_model("A"))
    K, T = syn.camera(H, W, 15.0)
    base_shift = [list(s) for s in model.shift]

    def frame(k, cached):
        f = [1.0, 2.5, 3.0, 1.0 + 0.75 * k]
        model.shift = [list(s) for s in base_shift]
        model.shift[3] = [base_shift[3][0] - 0.15 * k, base_shift[3][1] + 0.1 * k, base_shift[3][2]]
        rays = ops.generate_rays(K, T, H, W, frame_ids=f)
        model.view_key = view_key(K, T, H, W, f) if cached else None
        try:
            return render(model, rays)
        finally:
            model.view_key = None

    want = [frame(k, False) for k in range(3)]
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[1][0], want[2][0])
    cache = stnerf_amd.BackgroundCache()
    model.set_background_cache(cache)
    for k in range(3):
        got = frame(k, True)
        assert (cache.stats["hits"], cache.stats["misses"]) == (k * PIECES, PIECES), (k, cache.stats)
        assert_same_render(got, want[k], f"cached frame {k}")
    model.set_background_cache(None)


# ---- 4. opacity
def test_layer_alpha_neutral_tables_and_the_alpha_of_layer_two():
    model = make_model("A")
    l = model.total_layers
    rays = view_rays(model, True)
    plain = render(model, rays)
    for table in ([None] * l, [1.0] * l):
        model.layer_alpha = table
        assert_same_render(render(model, rays), plain, f"layer_alpha {table}")
    model.layer_alpha = None
    model.alpha = 0.3
    ref = render(model, rays)
    assert not torch.equal(ref[0], plain[0])
    model.alpha = 1
    model.layer_alpha = [1, 1, 0.3, None]
    assert_same_render(render(model, rays), ref, "layer_alpha [1, 1, 0.3] vs alpha 0.3")
    # the plain three-layer model, the issue's own [1, 1, a]
    model.clear_instances()
    model.layer_alpha = None
    model.alpha = 0.3
    rays3 = view_rays(model, True, frames=[1.0, 2.5, 3.0])
    ref3 = render(model, rays3)
    model.alpha = 1
    model.layer_alpha = [1, 1, 0.3]
    assert_same_render(render(model, rays3), ref3, "[1, 1, a] on the plain model")


@pytest.mark.parametrize("i", [1, 3])
def test_layer_alpha_zero_empties_that_layer_alone(i):
    model = edited(make_model("A"))
    l = model.total_layers
    rays = view_rays(model, True)
    plain = render(model, rays)
    assert bool(plain[2][:, i, 4].any()), "the layer is not on the picture"
    model.layer_alpha = [None] * l
    model.layer_alpha[i] = 0.0
    got = render(model, rays)
    assert not bool(bits(got[2][:, i, 0:3]).any()) and not bool(bits(got[2][:, i, 4]).any())
    for j in range(l):
        if j != i:
            assert_bit_equal(got[2][:, j], plain[2][:, j], f"layer_fine of layer {j}")
    assert_bit_equal(got[1], plain[1], "mixed_coarse")
    assert_bit_equal(got[3], plain[3], "layer_coarse")
    assert_bit_equal(got[4], plain[4], "mask")
    assert not torch.equal(got[0], plain[0])


def test_only_coarse_ignores_the_table():
    model = edited(make_model("A"))
    rays = view_rays(model, True)
    plain = render(model, rays, only_coarse=True)
    model.layer_alpha = [1.0, 0.0, 0.3, 0.5]
    assert_same_render(render(model, rays, only_coarse=True), plain, "only_coarse with a table")


# ---- 5. refusals, before any launch
@pytest.mark.parametrize("bad,exc,match", [
    ([1.0, -0.5, 1.0, 1.0], ValueError, "layer_alpha"),
    ([1.0, 1.0, float("nan"), 1.0], ValueError, "layer_alpha"),
    ([1.0, 1.0, 1.0, float("inf")], ValueError, "layer_alpha"),
    ([1.0, 1.0, 1.0], ValueError, "one entry per layer"),
])
def test_bad_opacity_tables_are_refused_before_any_launch(bad, exc, match):
    model = make_model("A")
    rays = view_rays(model, True)
    model.layer_alpha = bad
    ops.profile_begin()
    try:
        with pytest.raises(exc, match=match):
            render(model, rays)
    finally:
        launched = ops.profile_end()
    assert launched == [], launched
    if len(bad) == model.total_layers:                    # (refused by the library itself: its own error text)
        assert "layer_alpha[" in hip.last_error()


def test_layer_alpha_with_alpha_and_instances_in_training_are_refused():
    model = make_model("A")
    rays, rays3 = view_rays(model, True), view_rays(model, True, frames=[1.0, 2.5, 3.0])
    model.layer_alpha, model.alpha = [1.0] * 4, 0.5
    ops.profile_begin()
    try:
        with pytest.raises(ValueError, match="alpha"):
            render(model, rays)
        model.layer_alpha, model.alpha = None, 1
        model.train()
        with torch.enable_grad():
            assert any(p.requires_grad for p in model.parameters())
            with pytest.raises(NotImplementedError, match="instances"):
                model.render_rays_raw(rays, False, 0.0, 0.0, ref_chunk=CHUNK)
            model.clear_instances()
            model.layer_alpha = [1.0, 1.0, 1.0]
            with pytest.raises(NotImplementedError, match="layer_alpha"):
                model.render_rays_raw(rays3, False, 0.0, 0.0, ref_chunk=CHUNK)
    finally:
        launched = ops.profile_end()
        model.train(False)
    assert launched == [], launched
