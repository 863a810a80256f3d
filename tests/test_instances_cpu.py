"""Layer instances without a GPU: the model's bookkeeping (ids, refusals, the 16-layer cap, no new parameter), the host arithmetic
against the wide model of DESIGN.md section 7 (retimed boxes, pivot, ray transforms), the ray-width check, the renderer's
``duplicate_layer`` bookkeeping, ``render_pose``'s frame ids and the new C entry's declaration and export."""
import os
import re
import types

import pytest
import torch

from conftest import REPO
from stnerf_amd import hip, synthetic as syn

from instances_common import CASES, base_model, frame_ids, instance_edits, wide_model


def instanced(case):
    L, sources = CASES[case]
    model = base_model(L)
    ids = [model.add_instance(s) for s in sources]
    assert ids == list(range(L + 1, L + 1 + len(sources)))
    return model


def test_add_instance_ids_and_errors():
    model = base_model(2)
    assert model.instances == () and model.total_layers == 3
    assert model.add_instance(1) == 3 and model.add_instance(2) == 4 and model.add_instance(1) == 5
    assert model.instances == (1, 2, 1) and model.total_layers == 6 and model.layer_num == 2
    assert all(model.is_shown_layer(i) for i in range(6))
    for bad in (0, 3, 4, -1, 1.0, None):                      # the background, an instance as source, nonsense
        with pytest.raises(ValueError, match="performer"):
            model.add_instance(bad)
    assert model.instances == (1, 2, 1)
    model.hide_layer(4)
    assert not model.is_shown_layer(4)
    model.show_layer(4)
    assert model.is_shown_layer(4)
    model.clear_instances()
    assert model.instances == () and model.total_layers == 3 and sorted(model.display_layers) == [0, 1, 2]


def test_the_sixteen_layer_cap():
    model = base_model(2)
    for _ in range(13):
        model.add_instance(1)
    assert model.total_layers == hip.MAX_LAYERS == 16
    with pytest.raises(ValueError, match="STNERF_MAX_LAYERS"):
        model.add_instance(2)
    assert model.total_layers == 16


def test_an_instance_adds_no_parameter_and_no_state():
    model = base_model(2)
    keys, count = list(model.state_dict().keys()), sum(p.numel() for p in model.parameters())
    lists = [len(model.spacenets), len(model.spacenets_fine), len(model.time_deform_nets)]
    model.add_instance(2)
    model.add_instance(2)
    assert list(model.state_dict().keys()) == keys and sum(p.numel() for p in model.parameters()) == count
    assert [len(model.spacenets), len(model.spacenets_fine), len(model.time_deform_nets)] == lists and model.layer_num == 2
    assert model._module_index(1) == 0 and model._module_index(2) == 1 and model._module_index(3) == 1 and model._module_index(4) == 1


@pytest.mark.parametrize("case", ["A", "B", "L1"])
def test_host_arithmetic_matches_the_wide_model(case):
    model = instanced(case)
    L, K, l = model.layer_num, len(model.instances), model.total_layers
    model.scale, model.shift, model.rotation = instance_edits(l, L + 1)
    wide = wide_model(model)
    assert wide.layer_num == L + K and len(wide.spacenets) == L + K
    assert torch.equal(model._pivot(), wide._pivot())
    row0 = torch.tensor(frame_ids(L, K), dtype=torch.float32)
    (boxes, pivot), (boxes_w, pivot_w) = model._retimed_boxes(row0), wide._retimed_boxes(row0)
    assert boxes.shape == (l, 8, 3) and torch.equal(boxes, boxes_w) and torch.equal(pivot, pivot_w)
    for fine in (False, True):
        assert model._point_edits(l, fine) == wide._point_edits(l, fine)
    # the ray transforms: l entries, the same numbers; default centres from the expanded, edited table
    model.rotation = wide.rotation = [None] * (l - 1) + [0.4]
    tr, tr_w = model.layer_ray_transforms(boxes), wide.layer_ray_transforms(boxes_w)
    assert len(tr) == l and tr[:-1] == [None] * (l - 1)
    assert torch.equal(tr[-1][0], tr_w[-1][0]) and torch.equal(tr[-1][1], tr_w[-1][1])
    assert torch.equal(tr[-1][1], torch.mean(boxes[l - 1], 0))
    model.rotation = None
    assert model.layer_ray_transforms(None) == [None] * l
    model.rotation = [None] * (l - 1)                         # one entry per layer of l, not of layer_num + 1
    with pytest.raises(ValueError, match="one entry per layer"):
        model.layer_ray_transforms(boxes)


def test_ray_width_counts_the_instances():
    """Width 7 + L on a model with K = 1 is neither format: checked before anything else (the device check comes first, so
    the width check is reached through a tensor that claims to be on the GPU)."""
    model = instanced("A")

    class OnDevice(torch.Tensor):
        is_cuda = True

        def contiguous(self, *a, **k):
            return self

        def float(self):
            return self
    rays = torch.zeros(4, 7 + 2).as_subclass(OnDevice)
    with pytest.raises(ValueError, match="undefined ray format"):
        model.render_rays_raw(rays)
    with pytest.raises(ValueError, match="undefined ray format"):
        base_model(2).render_rays_raw(torch.zeros(4, 7 + 3).as_subclass(OnDevice))


def test_layer_alpha_checks_on_the_host():
    model = instanced("A")
    assert model.layer_alpha is None and model._layer_alpha_table() is None
    model.layer_alpha = [None, 0.5, None, 0]
    assert model._layer_alpha_table() == [1.0, 0.5, 1.0, 0.0]
    model.alpha = 0.5
    with pytest.raises(ValueError, match="alpha"):
        model._layer_alpha_table()
    model.alpha = 1
    model.layer_alpha = [1.0] * 3
    with pytest.raises(ValueError, match="one entry per layer"):
        model._layer_alpha_table()
    assert model._inference_only_edits() is not None
    model.layer_alpha = None
    assert "instances" in model._inference_only_edits()
    model.clear_instances()
    assert model._inference_only_edits() is None


def test_collective_fingerprint_covers_instances_and_opacity():
    from stnerf_amd.parallel import layers_fingerprint, packed_width, total_layers
    model = base_model(2)
    plain = layers_fingerprint(model)
    model.add_instance(2)
    one = layers_fingerprint(model)
    model.layer_alpha = [None, None, None, 0.5]
    ghost = layers_fingerprint(model)
    assert len(plain) == len(one) == len(ghost) and plain != one and one != ghost
    model.layer_alpha = [None, None, None, 0.25]
    assert layers_fingerprint(model) != ghost
    assert total_layers(model) == 4 and packed_width(total_layers(model), "fine") == 6 + 5 * 4
    assert total_layers(types.SimpleNamespace(layer_num=2)) == 3          # (a model without the notion: layer_num + 1)


# ---- the renderer
def make_renderer(model, frame_num=21, **kw):
    from stnerf_amd.render import LayeredNeuralRenderer
    K, T = syn.camera(17, 23, 15.0)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=model.layer_num, FRAME_NUM=frame_num, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]), OUTPUT_DIR="")
    return LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], **kw)


def test_duplicate_layer_bookkeeping():
    model = base_model(2)
    r = make_renderer(model)
    r.set_frame_duration(3, 13, 2)
    i = r.duplicate_layer(2, shift=[0.5, 0.0, 0.0], alpha=0.4)
    assert i == 3 and r.total_layers == 4 and model.instances == (2,) and r.layer_num == 2
    assert r.is_shown_layer(3) and model.is_shown_layer(3)
    assert r.min_frame == [1, 1, 3, 3] and r.max_frame == [21, 21, 13, 13]          # the copy starts with its source's span
    assert r.shift == model.shift == [[0.0, 0.0, 0.0]] * 3 + [[0.5, 0.0, 0.0]]
    assert r.layer_alpha == model.layer_alpha == [None, None, None, 0.4]
    assert r.scale is None and model.scale is None and r.rotation is None and model.rotation is None
    j = r.duplicate_layer(1, scale=0.8, rotation=(0.3, (0.0, 0.0, 0.0)))
    assert j == 4 and r.scale == model.scale == [1.0, 1.0, 1.0, 1.0, 0.8]
    assert r.rotation == model.rotation == [None, None, None, None, (0.3, (0.0, 0.0, 0.0))]
    assert r.shift[4] == [0.0, 0.0, 0.0] and r.layer_alpha == [None, None, None, 0.4, None]
    r.set_frame_duration(5, 9, 3)
    assert r.min_frame == [1, 1, 3, 5, 1] and r.max_frame == [21, 21, 13, 9, 21]
    r.set_path_fixed_gt_poses(0, 4)
    assert all(sorted(layer for layer, _ in pair) == [0, 1, 2, 3, 4] for pair in r.layer_frame_pairs)
    frames = lambda layer: [dict(pair)[layer] for pair in r.layer_frame_pairs]
    assert frames(3) == [5, 6, 7, 8, 9] and frames(2) == [3, 5, 8, 10, 13]
    source_before = frames(2)
    r.retime_by_key_frames(3, [9, 5], [6, 9])
    assert frames(2) == source_before and frames(3) != [5, 6, 7, 8, 9]
    with pytest.raises(RuntimeError, match="path setter"):
        r.duplicate_layer(1)
    assert model.instances == (2, 1)
    # render_path's per-layer lists have one entry per layer, instances included
    seen = []
    r.render_pose = lambda pose, K, pairs, *a, **k: seen.append(pairs) or (
        torch.zeros(17, 23, 3), torch.zeros(17, 23, 1), [torch.zeros(17, 23, 3)] * 5, [torch.zeros(17, 23, 1)] * 5)
    r.render_path()
    assert len(seen) == 4 and all(len(x) == 5 for x in (r.images_layer, r.depths_layer, r.images_scene, r.alphas_scene))
    assert all(len(x) == 4 for x in r.images_layer)


def test_schedules_have_one_entry_per_layer():
    model = base_model(2)
    r = make_renderer(model, s_shift=([[0.0, 0.0, 0.0]] * 3, [[0.1, 0.0, 0.0]] * 3))
    r.duplicate_layer(1)
    with pytest.raises(ValueError, match="s_shift"):                         # three entries, four layers
        r.set_path_fixed_gt_poses(0, 3)
    model = base_model(2)
    model.add_instance(1)
    r = make_renderer(model, s_shift=([[0.0, 0.0, 0.0]] * 4, [[0.0, 0.0, 0.0]] * 3 + [[0.4, 0.0, 0.0]]),
                      s_layer_alpha=([None, None, None, 1.0], [None, None, None, 0.0]))
    assert r.total_layers == 4 and r.layer_alpha == [None, None, None, 1.0] and model.layer_alpha == r.layer_alpha
    r.set_path_fixed_gt_poses(0, 5)
    assert r.s_layer_alpha_frame[2] == [None, None, None, 0.5] and r.s_layer_alpha_frame[4][3] == 0.0
    assert r.s_shift_frame[4][3] == [0.4, 0.0, 0.0]
    with pytest.raises(ValueError, match="s_layer_alpha"):
        make_renderer(base_model(2), s_layer_alpha=([None, 1.0, None], [None, 1.0, 0.5]))
    with pytest.raises(ValueError, match="s_layer_alpha"):
        make_renderer(base_model(2), s_layer_alpha=([None, 1.0], [None, 0.5])).set_path_fixed_gt_poses(0, 3)


def test_render_pose_hands_render_view_one_frame_id_per_layer(monkeypatch):
    import importlib
    rp = importlib.import_module("stnerf_amd.render.render_pose")     # (the module: the package re-exports the function under its name)
    model = instanced("B")
    seen = {}

    def fake_render_view(m, K, T, h, w, fids, *a, **k):
        seen["fids"] = list(fids)
        z3, z1 = torch.zeros(h * w, 3), torch.zeros(h * w, 1)
        layers = [(z3, z1, z1)] * m.total_layers
        return (z3, z1, z1), None, layers, None, None
    monkeypatch.setattr(rp, "render_view", fake_render_view)
    K, T = syn.camera(17, 23, 15.0)
    out = rp.render_pose(model, T, K, 17, 23, [(0, 1.0), (1, 2.0), (2, 3.0), (4, 7.0)], 20.0, device="cpu")
    assert seen["fids"] == [1.0, 2.0, 3.0, 0.0, 7.0]
    assert len(out[2]) == len(out[3]) == 5


# ---- the C ABI
def test_header_declares_and_library_exports_the_opacity_entry():
    header = open(os.path.join(REPO, "include", "stnerf.h")).read()
    decl = re.search(r"int\s+stnerf_render_rays_opacity\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/stnerf.h does not declare stnerf_render_rays_opacity"
    args = decl.group(1)
    assert "const float* layer_alpha_host" in args and "float* scene_out" in args and args.rstrip().endswith("stnerf_stream_t stream")
    assert "may ALIAS" in header
    assert "stnerf_render_rays_opacity" in hip.exported_symbols()
    if not os.path.exists(hip.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("stnerf_build", os.path.join(REPO, "st-nerf_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    lib = hip.lib()
    assert lib.stnerf_render_rays_opacity is not None
    # argument errors come back before any launch (no GPU here): null pointers
    import ctypes as C
    null = C.c_void_p(0)
    assert lib.stnerf_render_rays_opacity(null, 4, null, 0, None, None, null, null, null, 0, null, null, null, null, null, None, None,
                                          null, None, null) == hip.EINVAL
    assert "null pointer" in hip.last_error()
