"""MotionNet reuse (csrc/pipeline.hip): on the split-bf16 path a performer layer's MotionNet runs in launches of its own, over
the coarse points and then only over the fine samples whose depth is not one of the coarse depths; the others take the moved
coarse point.  The render must be bit-identical to the fused path (STNERF_MOTION_REUSE=0) -- all five outputs, every bit."""
import os
import types

import pytest
import torch

from stnerf_amd import ops, synthetic as syn

pytestmark = pytest.mark.gpu


def make_model(L, n1, n2, space_time=True, deform_time=True, seed=3):
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=deform_time,
                              USE_SPACE_TIME=space_time, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=n1, FINE_RAY_SAMPLING=n2)
    cfg = types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L))
    model = build_layered_model(cfg, camera_num=1)
    model.load_state_dict(syn.make_state_dict(L, space_time, deform_time, seed=seed))
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    return model.cuda().eval().set_precision("bf16x3")


def render(model, rays, reuse, **kw):
    """The five library outputs and the names of the profiled launches, with the switch set for this call only."""
    old = os.environ.get("STNERF_MOTION_REUSE")
    os.environ["STNERF_MOTION_REUSE"] = "1" if reuse else "0"
    try:
        model.seed = 11
        ops.profile_begin()
        with torch.no_grad():
            out = model.render_rays_raw(rays, **kw)
        torch.cuda.synchronize()
        names = [r["kernel"] for r in ops.profile_end()]
    finally:
        if old is None:
            os.environ.pop("STNERF_MOTION_REUSE")
        else:
            os.environ["STNERF_MOTION_REUSE"] = old
    return [o.clone() for o in out], names


def assert_bit_equal(model, rays, reused_layers, **kw):
    on, names_on = render(model, rays, True, **kw)
    off, names_off = render(model, rays, False, **kw)
    assert len(on) == len(off) == 5
    for k, (a, b) in enumerate(zip(on, off)):
        assert a.shape == b.shape and a.dtype == b.dtype, k
        # (bits, not values: NaN == NaN here, and -0 != +0)
        av = a.view(torch.uint8) if a.dtype == torch.uint8 else a.contiguous().view(torch.int32)
        bv = b.view(torch.uint8) if b.dtype == torch.uint8 else b.contiguous().view(torch.int32)
        assert torch.equal(av, bv), f"output {k}: {(av != bv).sum().item()} elements differ"
    # the fused path launches no MotionNet of its own; the reuse path two per reused layer and pipeline call
    calls = names_on.count("sample_coarse")
    assert "motionnet" not in names_off
    assert names_on.count("motionnet") == 2 * reused_layers * calls, names_on


@pytest.mark.parametrize("n1,n2", [(64, 64), (90, 30)])
def test_reuse_is_bit_identical_retimed(n1, n2):
    model = make_model(2, n1, n2)
    K, T = syn.camera(32, 48, 12.0)
    rays = ops.generate_rays(K, T, 32, 48, frame_ids=[1.0, 2.5, 1.0])      # retiming: one frame-id column per layer
    assert_bit_equal(model, rays, 2)


def test_reuse_is_bit_identical_without_retiming_and_in_reference_chunks():
    model = make_model(2, 64, 64)
    K, T = syn.camera(40, 64, 5.0)
    rays = ops.generate_rays(K, T, 40, 64, frame_ids=[2.5])
    assert_bit_equal(model, rays, 2)
    rays = ops.generate_rays(K, T, 40, 64, frame_ids=[1.0, 2.5, 1.5])
    assert_bit_equal(model, rays, 2, ref_chunk=512)


def test_hidden_layer_is_neither_deformed_nor_evaluated():
    model = make_model(3, 64, 64)
    model.hide_layer(2)
    K, T = syn.camera(32, 48, 8.0)
    rays = ops.generate_rays(K, T, 32, 48, frame_ids=[1.0, 2.5, 1.0, 2.0])
    assert_bit_equal(model, rays, 2)


def test_equal_edits_reuse_and_unequal_edits_fall_back():
    model = make_model(2, 64, 64)
    K, T = syn.camera(32, 48, 10.0)
    rays = ops.generate_rays(K, T, 32, 48, frame_ids=[1.0, 2.5, 1.0])
    # the same un-edit in both passes: both layers take the reuse path
    model.scale, model.shift = [1.0, 1.1, 0.9], [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.05, 0.0]]
    assert_bit_equal(model, rays, 2)
    # a None shift skips a layer's fine un-edit altogether (layered_rfrender.py:467-475) but not its coarse scale: layer 1's records
    # differ and it keeps the fused MotionNet, layer 2 is reused -- both in the same stage launches
    model.scale, model.shift = [1.0, 1.2, 0.9], [None, None, [0.05, 0.0, 0.0]]
    assert_bit_equal(model, rays, 1)


def test_rays_whose_coarse_depths_are_all_equal():
    """A performer slab 1e-3 thick, 2e4 away: the bins are wider than the hit threshold (1e-5) but the whole depth range is below
    one ulp of t, so the coarse depths of a ray are one or two values and every fine depth is one of them -- the slot lists are
    empty (all -1) and the MotionNet launch of the fine pass has no valid row."""
    model = make_model(1, 64, 64)
    bk = syn.aabb_corners((-3.0, -3.0, -3.0), (3.0, 3.0, 3.0)).reshape(1, 8, 3)
    per = torch.stack([syn.aabb_corners((-2e4, -2e4, 0.0), (2e4, 2e4, 1e-3)).reshape(1, 8, 3)] * 3, 0)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    K, T = syn.camera(16, 16, 0.0, dist=2e4)
    rays = ops.generate_rays(K, T, 16, 16, frame_ids=[1.0, 2.0])
    on, _ = render(model, rays, True)
    assert int(on[4][:, 1].ne(0).sum()) > 0, "no ray hits the slab"
    assert_bit_equal(model, rays, 1)
