"""Per-layer rotation, layer instances, the per-layer opacity table and the in-scene layer passes against the CPU oracle
(oracle/stnerf_oracle.py states all four since DESIGN.md section 7 was restated there), in fp32 and fp64.  The other GPU tests of
these features compare the kernels with themselves in another arrangement (rotated render == plain render of rotated rays,
instanced == wide, passes sum to the mix), which an error on both sides passes: an opacity entry on the wrong layer, a default
centre from the unedited box, an instance on its source's frame id, two passes swapped.  Here every output has an independent
expectation.  tests/test_oracle_scene_edits_cpu.py shows on the CPU that the comparison used (``assert_matches_oracle``) refuses
each of those errors and that every input of the base scene shows in what is compared.

Base scene: case A of instances_common (L = 2, one instance of performer 1), a 23 x 17 view (391 rays: no multiple of 64) at
orbit 15 degrees in launch pieces of 128 and reference chunks of 64, one frame id per layer, thresholds 0.05 / 0.02, the edits of
``instance_edits`` plus layer 1 turned by 0.4 about its DEFAULT centre, layer_alpha = [0.8, 0.6, 0.5, 0.35], draws replayed.
Bars: tests/test_gpu_render.py's, nothing new (``scene_edits_common.assert_matches_oracle``).  Measured figures:
profiles/scene_edits_oracle.md.  Needs an MI355X: `pytest -m gpu`."""
import pytest
import torch

import scene_edits_common as S
from instances_common import base_model
from stnerf_amd import ops, synthetic as syn

pytestmark = pytest.mark.gpu

_BASE = {}


def make_model(case, precision="bf16x3", schedule="stage"):
    """The case's model on the GPU in a known state (built and uploaded once per L), its draws replayed."""
    L = case["L"]
    if L not in _BASE:
        _BASE[L] = base_model(L).cuda()
    model = _BASE[L]
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.clear_instances()
    model.train(False)
    for src in case["sources"]:
        model.add_instance(src)
    model.coarse_ray_sample, model.fine_ray_sample = case["n1"], case["n2"]
    model.set_precision(precision)
    model.mlp_schedule = schedule
    model.max_rays_per_launch = S.CAP
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale, model.shift, model.rotation = case["scale"], case["shift"], case["rotation"]
    model.layer_alpha, model.alpha, model.near = case["layer_alpha"], case["alpha"], case["near"]
    for i in range(model.total_layers):
        (model.hide_layer if i in case["hidden"] else model.show_layer)(i)
    model.set_background_cache(None)
    jitter, u = S.case_draws(case)
    model.replay = {"jitter": jitter.cuda()}
    if not case["only_coarse"]:
        model.replay["u"] = u.cuda()
    return model


def coarse_depths(model, case, rays):
    """The sampler's depths (N,l,n1) of the render: ``ops.sample_coarse`` on every reference chunk with the tables the model hands
    the library for it (its edited boxes, pivot, point un-edits and ray transforms)."""
    l, out = model.total_layers, []
    edits = model._point_edits(l, False)
    for s in range(0, rays.shape[0], case["chunk"]):
        r = rays[s:s + case["chunk"]].contiguous()
        if r.shape[1] == 7:
            bb = model._box_table().to(r.device).float().index_select(0, r[:, 6].to(torch.int64) - 1)
            bk = model.bkgd_bbox.to(r.device).float().unsqueeze(0).expand(r.shape[0], 1, 8, 3)
            boxes, pivot = model._edit_boxes(torch.cat([bk, bb], 1).contiguous())
            rot = model._per_ray_box_transforms(r, boxes) if model.rotation is not None else None
        else:
            boxes, pivot = model._retimed_boxes(r[0, 6:].cpu())
            rot = model.layer_ray_transforms(boxes) if model.rotation is not None else None
            boxes = boxes.to(r.device)
        t, _, _ = ops.sample_coarse(r, boxes, case["n1"], jitter=model.replay["jitter"][:, s:s + case["chunk"]].contiguous(),
                                    edits=edits, pivot=pivot, want_xyz=False, rotations=rot)
        out.append(t)
    return torch.cat(out, 0)


def gpu_render(model, case, rays):
    with torch.no_grad():
        out = model.render_rays_scene(rays, case["only_coarse"], case["thr"], case["bthr"], ref_chunk=case["chunk"])
        t = coarse_depths(model, case, rays)
    torch.cuda.synchronize()
    l = model.total_layers
    assert len(out[1]) == l and len(out[0][2]) == len(out[0][3]) == len(out[0][4]) == l
    return S.flat(out, t)


def report(name, figures):
    """One line per case for profiles/scene_edits_oracle.md, every figure as HIP / fp32 oracle: rays above the tolerance against
    fp64 and the largest median / 90th percentile of that error over the fine outputs and over the passes; the worst coarse error."""
    fine = {k: v for k, v in figures.items() if isinstance(v, tuple)}
    coarse = [v for v in figures.values() if not isinstance(v, tuple)]
    line = f"{name}:"
    for tag in ("fine_mixed", "fine_layer", "scene"):
        rows = [v for k, v in fine.items() if k.startswith(tag)]
        if rows:
            line += (f" {tag} outliers {sum(r[0] for r in rows)} / {sum(r[1] for r in rows)} (worst {max(r[0] for r in rows)} / "
                     f"{max(r[1] for r in rows)}), p50 {max(r[4] for r in rows):.2e} / {max(r[5] for r in rows):.2e}, "
                     f"p90 {max(r[6] for r in rows):.2e} / {max(r[7] for r in rows):.2e};")
    if coarse:
        line += f" coarse-stage max abs err {max(coarse):.2e}"
    print(line)


def run_case(name, case, precision="bf16x3", schedule="stage"):
    rays = S.case_rays(case)
    ref32, ref64 = S.oracle_render(case, rays), S.oracle_render(case, rays, torch.float64)
    model = make_model(case, precision, schedule)
    got = gpu_render(model, case, rays.cuda())
    report(f"{name} {precision}/{schedule}", S.assert_matches_oracle(got, ref32, ref64, case["only_coarse"], name))
    return got, ref32, model


def zero_bits(x):
    return not bool(x.contiguous().view(torch.int32).any())


@pytest.mark.parametrize("precision,schedule", [("bf16x3", "stage"), ("fp32", "stage"), ("fp32", "per_net")])
def test_base_scene(precision, schedule):
    got, ref32, model = run_case("base", S.make_case(), precision, schedule)
    assert model.instances == (1,) and model.total_layers == 4
    assert all(int(got[f"mask{i}"].sum()) >= 0.2 * S.N for i in range(4))


@pytest.mark.parametrize("n1,n2,near", [(8, 0, 0.0), (12, 6, 4.0)])
def test_only_coarse_ignores_the_table_and_takes_its_passes_from_the_coarse_stage(n1, n2, near):
    """(8, 0, near 0): the coarse stage cuts no background density (no threshold acts on it there), so the background covers
    the performers and their passes stay below 0.02 -- still 400 times the bar.  (12, 6, near 4.0): the background in front of
    the performers is cut, and every performer's pass shows (the oracle counts 75 / 148 / 31 rays with a pass alpha above 0.01)."""
    case = S.make_case(n1=n1, n2=n2, only_coarse=True, near=near)
    got, ref32, _ = run_case(f"only_coarse {n1}+{n2}, near {near}", case)
    assert torch.equal(got["fine_mixed"], got["coarse_mixed"])
    if near == 0:
        assert int((got["scene0"][:, 4] > 0.5).sum()) >= 0.8 * S.N
    else:
        assert all(int((got[f"scene{i}"][:, 4] > 0.01).sum()) >= 20 for i in (1, 2, 3))


def test_sixty_four_coarse_and_sixty_four_fine_samples():
    run_case("64+64", S.make_case(n1=64, n2=64))


def test_rays_with_one_frame_id():
    """Rays 7 wide: every layer, the instance too, takes the ray's one frame id; the default centre is row 0's box's."""
    case = S.make_case(frame=2.0)
    assert S.case_rays(case).shape == (S.N, 7)
    run_case("width-7 rays", case)


def test_two_reference_chunk_groups_each_with_its_own_default_centre():
    """The frame ids change at ray 256: layer 1's box, and with it the default centre of its rotation, is another one there."""
    ids = S.make_case()["groups"][0][1]
    other = [1.0, 1.5, 2.0, 3.0]
    assert other[1] != ids[1]
    case = S.make_case(groups=[(0, ids), (256, other)])
    rays = S.case_rays(case)
    assert float(rays[255, 7]) == ids[1] and float(rays[256, 7]) == other[1]
    got, ref32, model = run_case("two chunk groups", case)
    c0 = model.layer_ray_transforms(model._retimed_boxes(rays[0, 6:])[0])[1][1]
    c1 = model.layer_ray_transforms(model._retimed_boxes(rays[256, 6:])[0])[1][1]
    assert float((c0 - c1).abs().max()) >= 0.04


def test_rotated_background_with_a_near_cut():
    """The background box scaled past the camera and turned: its near hit is behind the ray origin, so the ``layer == 0 &&
    start <= 0`` clamp acts on the turned ray, and ``near`` cuts into its depths."""
    base = S.make_case()
    rotation, scale = list(base["rotation"]), list(base["scale"])
    rotation[0], scale[0] = 0.3, 1.5
    case = S.make_case(rotation=rotation, scale=scale, near=1.5)
    got, ref32, _ = run_case("background rotated", case)
    first = ref32["t_coarse"][:, 0, 0]
    assert float(first.min()) >= 0.0 and float(first.max()) < 1.0 and float(first.min()) < case["near"]     # clamped starts


def test_hidden_rotated_instance():
    case = S.make_case(hidden=(3,))
    got, ref32, _ = run_case("instance hidden", case)
    for k in ("scene3", "fine_layer3", "coarse_layer3"):
        assert zero_bits(got[k]), f"{k} of the hidden layer"
    assert int(got["mask3"].sum()) >= 0.2 * S.N                   # (its rays are still marked: the reference's mask)


def test_render_pose_scene_passes():
    """Through ``render_pose(scene_passes=True)``: a view of less than one ``layered_batchify_ray`` chunk, so one reference chunk
    and the model's default thresholds; rays generated on the device (the oracle gets those)."""
    from stnerf_amd.render.render_pose import render_pose
    case = S.make_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids, far = case["groups"][0][1], 20.0
    K, T = syn.camera(S.H, S.W, case["orbit"])
    rays = ops.generate_rays(K, T, S.H, S.W, frame_ids=ids).cpu()
    ref32, ref64 = S.oracle_render(case, rays, chunked=False), S.oracle_render(case, rays, torch.float64, chunked=False)
    model = make_model(case)
    l = model.total_layers
    color, depth, color_layer, depth_layer, passes = render_pose(model, T, K, S.H, S.W, list(enumerate(ids)), far, 0.05, 0.02,
                                                                 scene_passes=True)
    torch.cuda.synchronize()
    assert sorted(passes) == ["alpha_scene", "color_scene", "depth_scene"] and all(len(v) == l for v in passes.values())
    flat = lambda img: img.reshape(S.N, -1).cpu()
    got = {f"scene{i}": torch.cat([flat(passes["color_scene"][i]), flat(passes["depth_scene"][i]) * far,
                                   flat(passes["alpha_scene"][i])], 1) for i in range(l)}
    keep = lambda d: {k: d[k] for k in got}
    report("render_pose", S.assert_matches_oracle(got, keep(ref32), keep(ref64), False, "render_pose"))
    S.fine_stage_bar(flat(color), ref32["fine_mixed"][:, 0:3], ref64["fine_mixed"][:, 0:3], S.COLOR_ATOL, "render_pose colour")
    assert color.shape == (S.H, S.W, 3) and passes["depth_scene"][0].shape == (S.H, S.W, 1)
