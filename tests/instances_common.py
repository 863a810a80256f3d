"""Shared by tests/test_gpu_instances.py and tests/test_instances_cpu.py: the synthetic instanced model M and its WIDE model W(M)
(DESIGN.md section 7): LAYER_NUM = L + K, the source's modules and box column copied for every instance, every other setting the
same, the per-layer lists given per layer of l = 1 + L + K."""
import types

import torch

from stnerf_amd import synthetic as syn

# the cases of GPU test 1: name -> (L, sources)
CASES = {"A": (2, (1,)), "B": (2, (2, 2)), "L1": (1, (1,))}
CENTRE = (0.1, -0.2, 0.05)
# make_state_dict's seed.  The random density heads leave many a synthetic performer empty (sigma <= 0 on every sample), and an
# empty layer composites to zeros whatever its network is: seed 4 is the first for which the CPU oracle finds every layer of the
# L = 2 and the L = 1 scene opaque on a third of its hit rays or more, in the coarse and in the fine pass
SEED = 4


def cfg_of(layer_num):
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    return types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=layer_num))


def base_model(L):
    """The L-performer synthetic model with its boxes (on the CPU, eval mode, no instance)."""
    from stnerf_amd.modeling import build_layered_model
    model = build_layered_model(cfg_of(L), camera_num=1)
    model.load_state_dict(syn.make_state_dict(L, True, True, seed=SEED))
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    return model.eval()


def wide_state_dict(model):
    """W(M)'s state dict: M's, plus a copy of the source's tensors under every instance's module index."""
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    L = model.layer_num
    for j, src in enumerate(model.instances):
        for lst in ("spacenets", "spacenets_fine", "time_deform_nets"):
            head = f"{lst}.{src - 1}."
            for k in [k for k in sd if k.startswith(head)]:
                sd[f"{lst}.{L + j}." + k[len(head):]] = sd[k].clone()
    return sd


def wide_model(model):
    """W(M), freshly built on M's device, with M's render settings (``sync_settings``)."""
    from stnerf_amd.modeling import build_layered_model
    L, K = model.layer_num, len(model.instances)
    wide = build_layered_model(cfg_of(L + K), camera_num=1)
    wide.load_state_dict(wide_state_dict(model))
    wide = wide.to(next(model.parameters()).device).eval()
    return sync_settings(model, wide)


def sync_settings(model, wide):
    """Give W(M) the settings M has now: the boxes (instance columns copied from the sources'), the per-layer lists as they are
    and every scalar knob."""
    bb = model.bboxes
    wide.set_bkgd_bbox(model.bkgd_bbox)
    wide.set_bboxes(torch.cat([bb] + [bb[:, s - 1:s].clone() for s in model.instances], 1))
    for name in ("coarse_ray_sample", "fine_ray_sample", "mlp_schedule", "max_rays_per_launch", "seed", "fresh_draws_per_call",
                 "scale", "shift", "rotation", "near", "alpha", "layer_alpha", "boarder_weight"):
        setattr(wide, name, getattr(model, name))
    wide.set_precision(model.bkgd_spacenet.precision)
    wide.display_layers = dict(model.display_layers)
    assert wide.layer_num + 1 == model.total_layers and wide.instances == ()
    return wide


def instance_edits(l, first_instance):
    """Per-layer scale / shift / rotation lists of l entries: the performers lightly edited, every instance with a shift, a scale
    and a (rotation, centre) of its own."""
    scale, shift, rotation = [1.0] * l, [[0.0, 0.0, 0.0] for _ in range(l)], [None] * l
    if first_instance > 1:
        scale[1], shift[1] = 1.1, [0.05, 0.0, 0.0]
    for k, i in enumerate(range(first_instance, l)):
        scale[i] = 0.9 - 0.1 * k
        shift[i] = [0.35 + 0.2 * k, -0.3 + 0.5 * k, 0.05]
        rotation[i] = (0.6 - 1.1 * k, CENTRE)
    return scale, shift, rotation


def frame_ids(L, K):
    """One frame id per layer (the synthetic boxes have frames 1..3): the instances' differ from their sources'."""
    performers = [2.5, 3.0][:L]
    return [1.0] + performers + [1.5, 2.0, 1.0][:K]
