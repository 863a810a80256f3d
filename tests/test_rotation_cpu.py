"""Per-layer rotation, host side (no GPU): the spec parser of ``LayeredRFRender.rotation`` (angle / matrix / pair / None entries,
refusals), the numbers ``layer_ray_transforms`` hands to the library (m = R^T, default centre = the edited box's corner mean), the
ctypes mirror of stnerf_layer_rotation against the C compiler, the background cache key (layer 0's rotation only), the renderer's
forwarding and ``s_rotation`` schedule, the argument checks of the new entries, and the training path's refusal."""
import ctypes as C
import math
import os
import shutil
import subprocess
import types

import pytest
import torch

from conftest import REPO
from stnerf_amd import hip, synthetic as syn
from stnerf_amd.bkgd_cache import view_key


def make_model(L=2):
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
    return model.eval()


def frame0_boxes(model):
    return torch.cat([model.bkgd_bbox.float(), model.bboxes[0].float()], 0)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=torch.float64)


def test_default_is_no_rotation():
    model = make_model()
    assert model.rotation is None
    assert model.layer_ray_transforms(frame0_boxes(model)) == [None, None, None]
    model.rotation = [None, None, None]
    assert model.layer_ray_transforms(None) == [None, None, None]


def test_angle_matrix_pair_and_none_entries():
    model = make_model()
    boxes = frame0_boxes(model)
    R = rot_z(0.3) @ rot_x(-0.2)
    model.rotation = [None, 0.6, (R, [0.5, -0.25, 0.125])]
    tr = model.layer_ray_transforms(boxes)
    assert tr[0] is None
    m1, c1 = tr[1]
    assert m1.dtype == torch.float32 and tuple(m1.shape) == (3, 3) and c1.dtype == torch.float32 and tuple(c1.shape) == (3,)
    # the angle's matrix: built in fp64, rounded to fp32, transposed
    assert torch.equal(m1, rot_z(0.6).to(torch.float32).T)
    # default centre: the fp32 mean of the box's eight corners -- layer 1 of the synthetic scene: x in [-1.2, -0.12], y, z in [-1, 1]
    assert torch.equal(c1, torch.mean(boxes[1], 0))
    assert torch.allclose(c1, torch.tensor([-0.66, 0.0, 0.0]), atol=1e-6)
    m2, c2 = tr[2]
    assert torch.equal(m2, R.to(torch.float32).T) and torch.equal(c2, torch.tensor([0.5, -0.25, 0.125]))
    # a bare matrix, a pair with an angle, numpy input
    model.rotation = [R.numpy(), (0.6, (1.0, 2.0, 3.0)), None]
    tr = model.layer_ray_transforms(boxes)
    assert torch.equal(tr[0][0], R.to(torch.float32).T) and torch.equal(tr[0][1], torch.mean(boxes[0], 0))
    assert torch.equal(tr[1][0], m1) and torch.equal(tr[1][1], torch.tensor([1.0, 2.0, 3.0])) and tr[2] is None
    # explicit centres need no box
    model.rotation = [None, (0.6, (1.0, 2.0, 3.0)), None]
    assert torch.equal(model.layer_ray_transforms(None)[1][0], m1)


def test_quarter_turn_about_z_is_counter_clockwise_seen_from_above():
    model = make_model()
    model.rotation = [None, math.pi / 2, None]
    m, _ = model.layer_ray_transforms(frame0_boxes(model))[1]
    # the layer sees the ray turned BACK: the world's +x is the layer's -y
    assert float((m @ torch.tensor([1.0, 0.0, 0.0]) - torch.tensor([0.0, -1.0, 0.0])).abs().max()) <= 1e-7
    assert float((m @ torch.tensor([0.0, 0.0, 1.0]) - torch.tensor([0.0, 0.0, 1.0])).abs().max()) == 0.0


def test_default_centre_follows_the_edited_box():
    model = make_model()
    model.scale, model.shift = [1.0, 1.5, 1.0], [[0.0, 0.0, 0.0], [0.25, -0.5, 0.125], None]
    model.rotation = [None, 0.6, 0.2]
    edited, _ = model._edit_boxes(frame0_boxes(model).clone())
    tr = model.layer_ray_transforms(edited)
    for i in (1, 2):
        assert torch.equal(tr[i][1], torch.mean(edited[i], 0))
    assert not torch.equal(tr[1][1], torch.mean(frame0_boxes(model)[1], 0))


def test_refusals():
    model = make_model()
    boxes = frame0_boxes(model)
    model.rotation = [None, 0.6]
    with pytest.raises(ValueError, match="one entry per layer"):
        model.layer_ray_transforms(boxes)
    for bad in (rot_z(0.3) * 1.01,                                          # a scaling: depths would change
                torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)),     # a reflection: det < 0
                torch.tensor([[1.0, 0.1, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)):   # a shear
        model.rotation = [None, bad, None]
        with pytest.raises(ValueError, match="not a rotation"):
            model.layer_ray_transforms(boxes)
    model.rotation = [None, rot_z(0.3) * (1.0 + 1e-7), None]               # (inside the 1e-5 bound: fp32 rounding of a rotation)
    assert model.layer_ray_transforms(boxes)[1] is not None
    model.rotation = [None, [1.0, 2.0, 3.0], None]
    with pytest.raises(ValueError, match="angle, a 3x3 matrix"):
        model.layer_ray_transforms(boxes)
    model.rotation = [None, (0.6, [1.0, 2.0]), None]
    with pytest.raises(ValueError, match="3 coordinates"):
        model.layer_ray_transforms(boxes)
    model.rotation = [None, 0.6, None]
    with pytest.raises(ValueError, match="no centre"):
        model.layer_ray_transforms(None)


def test_mixed_frame_ids_need_an_explicit_centre():
    """Width-7 rays carry per-ray boxes: without a centre the rays must share one frame id."""
    model = make_model()
    rays = torch.zeros(8, 7)
    rays[:, 6] = 1.0
    fid = rays[:, 6].to(torch.int64) - 1
    per_ray = torch.cat([model.bkgd_bbox.float().unsqueeze(0).expand(8, 1, 8, 3), model.bboxes.float().index_select(0, fid)], 1)
    model.rotation = [None, 0.6, None]
    tr = model._per_ray_box_transforms(rays, per_ray)
    assert torch.equal(tr[1][1], torch.mean(per_ray[0, 1], 0))
    rays[2, 6] = 2.0
    with pytest.raises(ValueError, match="mix frame ids"):
        model._per_ray_box_transforms(rays, per_ray)
    model.rotation = [None, (0.6, [0.0, 0.0, 0.0]), None]                           # an explicit centre: no box needed, no check
    assert torch.equal(model._per_ray_box_transforms(rays, per_ray)[1][1], torch.zeros(3))


def test_rotation_struct_matches_the_header(tmp_path):
    assert C.sizeof(hip.LayerRotation) == 52
    assert [getattr(hip.LayerRotation, f).offset for f, _ in hip.LayerRotation._fields_] == [0, 36, 48]
    assert hip.StageLayer._fields_[-1][0] == "rotation" and hip.StageLayer.rotation.offset == 64 and C.sizeof(hip.StageLayer) == 72
    gcc = shutil.which("gcc")
    if gcc is None:
        return                                   # (the constants above are the x86-64 / LP64 layout of the header's structs)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){']
    for cname, cls in (("stnerf_layer_rotation", hip.LayerRotation), ("stnerf_stage_layer", hip.StageLayer)):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in (("stnerf_layer_rotation", hip.LayerRotation), ("stnerf_stage_layer", hip.StageLayer)):
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"


def test_new_entries_are_exported_and_check_their_arguments():
    lib = hip.lib()
    names = ("stnerf_sample_coarse_rot", "stnerf_resample_rot", "stnerf_rgb_ray_bias_rot", "stnerf_spacenet_fwd_rot", "stnerf_render_rays_rot")
    header = open(os.path.join(REPO, "include", "stnerf.h")).read()
    for name in names:
        assert name in hip.exported_symbols() and getattr(lib, name) is not None and name + "(" in header
    null, fake = C.c_void_p(0), 1 << 20
    rot = (hip.LayerRotation * 3)()
    rot[1].enabled = 1
    assert lib.stnerf_sample_coarse_rot(null, 4, 9, null, 0, 3, 8, null, 0, 0, 0, 0, None, None, rot, null, null, null, null) == hip.EINVAL
    assert lib.stnerf_sample_coarse_rot(fake, 0, 9, fake, 0, 3, 8, null, 0, 0, 0, 0, None, None, rot, fake, null, fake, null) == hip.OK
    assert lib.stnerf_resample_rot(null, null, 4, 3, 12, 6, null, 0, 0, 0, 0, null, 9, None, None, rot, null, null, null, null, null, null,
                                   null) == hip.EINVAL
    assert lib.stnerf_resample_rot(fake, fake, 0, 3, 12, 6, null, 0, 0, 0, 0, fake, 9, None, None, rot, null, fake, null, null, null, null,
                                   null) == hip.OK
    assert lib.stnerf_rgb_ray_bias_rot(7, null, 1, null, null, null, 0, null, 0, null, rot, null) == hip.EINVAL and "bad kind" in hip.last_error()
    assert lib.stnerf_rgb_ray_bias_rot(hip.NET_SPACE, fake, 0, null, null, fake, 3, null, 0, fake, rot, null) == hip.OK
    assert lib.stnerf_spacenet_fwd_rot(7, null, 1, 1, null, null, null, 0, null, 0, null, 0, null, 0, null, rot, null) == hip.EINVAL
    assert lib.stnerf_render_rays_rot(null, 4, null, 0, None, None, null, null, null, 0, null, null, null, null, null, None, rot, null) == hip.EINVAL
    from stnerf_amd import ops
    with pytest.raises(ValueError, match="one entry per layer"):
        ops._rotations([None, (torch.eye(3), torch.zeros(3))], 3)
    assert ops._rotations([None, None, None], 3) is None and ops._rotations(None, 3) is None
    arr = ops._rotations([None, (rot_z(0.6).to(torch.float32).T, torch.tensor([1.0, 2.0, 3.0])), None], 3)
    assert [arr[i].enabled for i in range(3)] == [0, 1, 0] and list(arr[1].centre) == [1.0, 2.0, 3.0]
    assert list(arr[1].m) == rot_z(0.6).to(torch.float32).T.reshape(-1).tolist()


def key_of(model, frame_ids=(1.0, 1.0, 1.0)):
    K, T = syn.camera(17, 23, 15.0)
    return model.background_cache_key(view_key(K, T, 17, 23, list(frame_ids)), (0, 128), (0, 0, 0), True, False)


def test_cache_key_reacts_to_layer_zero_rotation_only():
    model = make_model()
    base = key_of(model)
    model.rotation = [None, None, None]
    assert key_of(model) == base
    model.rotation = [None, 0.6, (rot_z(0.2) @ rot_x(0.1), [0.0, 0.5, 0.0])]        # performers: a sweep over them must hit
    assert key_of(model) == base
    model.rotation = [None, -1.3, None]
    assert key_of(model) == base
    model.rotation = [0.1, None, None]
    k1 = key_of(model)
    assert k1 != base and k1[1] == base[1]
    model.rotation = [0.1, 0.6, None]
    assert key_of(model) == k1
    model.rotation = [0.2, 0.6, None]
    k2 = key_of(model)
    assert k2 not in (base, k1)
    model.rotation = [(0.2, [0.0, 0.0, 1.0]), 0.6, None]                              # the centre is part of it
    assert key_of(model) not in (base, k1, k2)
    model.rotation = None
    assert key_of(model) == base


def test_renderer_forwards_rotation_and_builds_the_schedule():
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    model = make_model()
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = syn.camera(17, 23, 15.0)
    rotation = [None, 0.6, None]
    r = LayeredNeuralRenderer(cfg, None, None, rotation, model=model, gt_poses=T[None], gt_Ks=[K])     # the reference's fourth positional
    assert r.rotation is rotation and model.rotation is rotation
    assert LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K]).model.rotation is None
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], s_rotation=([None, 0.0, 0.5], [None, 1.0, -0.5]))
    assert model.rotation == [None, 0.0, 0.5]
    r.set_path_fixed_gt_poses(0, 5)
    assert len(r.s_rotation_frame) == 5
    for i, row in enumerate(r.s_rotation_frame):
        assert row[0] is None and row[1] == 0.0 + i * (1.0 / 4) and row[2] == 0.5 + i * (-1.0 / 4)
    with pytest.raises(ValueError, match="s_rotation"):
        LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], s_rotation=([None, 0.0, 0.5], [0.1, 1.0, -0.5]))
    with pytest.raises(TypeError):
        LayeredNeuralRenderer(cfg, None, None, None, None, None, None, False, ([0.0], [1.0]))          # keyword-only


def test_training_path_refuses_a_rotation():
    from stnerf_amd.modeling.training import render_rays_train
    model = make_model()
    model.rotation = [None, 0.6, None]
    rays = torch.zeros(4, 9)
    with pytest.raises(NotImplementedError, match="render-time edit"):
        render_rays_train(model, rays, frame0_boxes(model), None, True, False, 0.0, 0.0, (0, 0, 0), None)
    model.rotation = [None, None, None]                                              # nothing set: the check lets the call through
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_rays_train(model, rays, frame0_boxes(model), None, True, False, 0.0, 0.0, (0, 0, 0), None)
