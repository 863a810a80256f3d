"""Depth-tested occluder compositing without a GPU (include/stnerf.h / DESIGN.md sections 4.2 and 7): the conditions the oracle
case must meet before tests/test_gpu_occluder.py compares anything with it, the identities of the numpy restatement, that the
comparison refuses three deliberate errors of the definition, ``ops.ray_parameter`` against its definition, the Python refusals,
and that the header, the prototypes and the library agree on the new entries."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import stnerf_oracle as O
from stnerf_amd import hip, ops, synthetic as syn

import occluder_common as OC
import scene_edits_common as S

HEADER = open(os.path.join(REPO, "include", "stnerf.h")).read()
NEW = ("stnerf_scene_occluder", "stnerf_occluder_stop", "stnerf_render_rays_occluded")
F = np.float32


@pytest.fixture(scope="module")
def oracles():
    case, occ = OC.oracle_case(), OC.case_occluder()
    return case, occ, OC.oracle_occluded(case, occ), OC.oracle_occluded(case, occ, torch.float64)


# ---------------------------------------------------------------------------------------- conditions on the oracle alone
def test_oracle_case_meets_the_conditions_of_the_comparison(oracles):
    case, occ, (ref32, info32), (ref64, info64) = oracles
    keep, figures = OC.oracle_conditions(info32, info64, occ)
    print(figures)
    ap, present = OC.np_present(occ)
    assert int(present.sum()) == int((np.arange(S.N) % 3 != 2).sum()) and set(ap.tolist()) == {0.0, 0.5, 1.0}
    assert figures["left_out"] <= OC.MAX_LEFT_OUT * S.N and min(figures["split"]) >= OC.MIN_SPLIT_RAYS
    # the occluder sits inside the scene: on many rays part of the scene is in front of it and part behind
    front_alpha = sum((torch.where(info32["behind"][:, i], 0.0, info32["merged_weights"][:, i].double())).sum(1) for i in range(4))
    assert int(((front_alpha > 0.05) & (front_alpha < 0.95)).sum()) >= 100
    # and it shows: the occluded mix differs from the plain one on present rays, and is the plain one on absent rays
    plain = S.oracle_render(case)["fine_mixed"]
    diff = (ref32["fine_occluded_mixed"] - plain).abs().amax(1)
    assert bool((diff[torch.from_numpy(~present)] == 0).all()) and int((diff[torch.from_numpy(present)] > 1e-2).sum()) >= 100
    OC.assert_occluded_matches_oracle(ref32, ref32, ref64, keep, "fp32 oracle against itself")


@pytest.mark.parametrize("wrong", ["q_front", "T_whole"])
def test_the_comparison_refuses_a_wrong_mix(oracles, wrong):
    case, occ, (ref32, info32), (ref64, info64) = oracles
    keep, _ = OC.oracle_conditions(info32, info64, occ)
    bad, _ = OC.oracle_occluded(case, occ, wrong=wrong)
    with pytest.raises(AssertionError):
        OC.assert_occluded_matches_oracle(bad, ref32, ref64, keep, wrong)


def test_the_comparison_refuses_gt_in_place_of_ge_at_a_depth_equal_to_z(oracles):
    """z = exactly the depth of each ray's heaviest sample (the fp32 oracle's): that sample is behind.  Both sides are evaluated
    in fp32 on the same depths (an fp64 oracle has other depths, so no tie), the right one standing in for the exact result."""
    case, occ, (_, info32), _ = oracles
    w, t = info32["merged_weights"].flatten(1), info32["t_fine"].flatten(1)
    k = w.argmax(1, keepdim=True)
    tie = occ.copy()
    tie[:, 4] = t.gather(1, k).squeeze(1).numpy()
    tie[:, 3] = 1.0
    assert float(w.gather(1, k).median()) > 0.05
    right, info = OC.oracle_occluded(case, tie)
    assert bool(info["behind"].flatten(1).gather(1, k).all())
    wrong, _ = OC.oracle_occluded(case, tie, wrong="gt")
    keep = torch.ones(S.N, dtype=torch.bool)
    OC.assert_occluded_matches_oracle(right, right, right, keep, "tie, right")
    with pytest.raises(AssertionError):
        OC.assert_occluded_matches_oracle(wrong, right, right, keep, "tie, wrong")


# ---------------------------------------------------------------------------------------- identities of the restatement
def _random_case(n=40, l=3, seed=0):
    g = np.random.default_rng(seed)
    front, behind = (g.random((n, l, 5)) * 0.2).astype(F), (g.random((n, l, 5)) * 0.2).astype(F)
    scene, mixed = g.random((n, l, 5)).astype(F), g.random((n, 5)).astype(F)
    occ = np.concatenate([g.random((n, 3)), g.choice([0.0, -1.0, np.nan, 0.5, 1.0, 2.0], (n, 1)),
                          g.choice([np.nan, np.inf, -np.inf, 1.0, 3.0, -2.0], (n, 1))], 1).astype(F)
    return front, behind, scene, mixed, occ


def test_absent_rows_give_the_plain_outputs():
    front, behind, scene, mixed, occ = _random_case()
    ap, present = OC.np_present(occ)
    a, z = occ[:, 3], occ[:, 4]
    want = np.isin(a, [0.5, 1.0, 2.0]) & np.isin(z, [1.0, 3.0, -2.0])
    assert np.array_equal(present, want) and 5 <= present.sum() <= 35
    assert set(ap[present].tolist()) == {0.5, 1.0} and not ap[~present & ~np.isfinite(a)].any()
    om, osc, share = OC.np_mix(front, behind, occ, scene, mixed)
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    assert np.array_equal(bits(om[~present]), bits(mixed[~present])) and np.array_equal(bits(osc[~present]), bits(scene[~present]))
    assert not bits(share[~present]).any()
    f, b = OC.np_front_behind(occ, scene)
    assert np.array_equal(bits(f[~present]), bits(scene[~present])) and not bits(b[~present]).any()
    assert not np.array_equal(om[present], mixed[present])


def test_the_shares_sum_to_the_occluded_mix():
    front, behind, scene, mixed, occ = _random_case(seed=1)
    om, osc, share = OC.np_mix(front, behind, occ, scene, mixed)
    _, present = OC.np_present(occ)
    total = osc.astype(np.float64).sum(1) + share
    assert np.abs(total - om)[present].max() <= 8 * np.finfo(F).eps * np.abs(total[present]).max()


def test_an_opaque_occluder_behind_everything_adds_what_the_scene_lets_through():
    front, _, scene, mixed, occ = _random_case(seed=2)
    occ[:, 3], occ[:, 4] = 1.0, 50.0
    om, osc, share = OC.np_mix(front, np.zeros_like(front), occ, scene, mixed)
    assert np.array_equal(osc, front)                      # pass_i = front_i + 0 * 0
    T = np.maximum(F(1) - ((front[:, 0, 4] + front[:, 1, 4]).astype(F) + front[:, 2, 4]).astype(F), F(0))
    x = np.concatenate([occ[:, 0:3], occ[:, 4:5], np.ones((len(occ), 1), F)], 1)
    assert np.array_equal(share, (T[:, None] * x).astype(F))
    assert np.array_equal(om, (((front[:, 0] + front[:, 1]).astype(F) + front[:, 2]).astype(F) + share).astype(F))
    # a translucent one lets the scene behind it through in proportion: q = 1 - a
    occ[:, 3] = 0.25
    _, osc, _ = OC.np_mix(np.zeros_like(front), front, occ, scene, mixed)
    assert np.array_equal(osc, (F(0.75) * front).astype(F))


def test_the_stop_rule():
    occ = np.array([[0, 0, 0, 1.0, 2.0], [0, 0, 0, 1.0, 5.0], [0, 0, 0, 1.0, 3.0], [0, 0, 0, np.nextafter(F(1), F(0)), 2.0],
                    [0, 0, 0, 2.0, 2.0], [0, 0, 0, 1.0, np.nan], [0, 0, 0, 1.0, -np.inf], [0, 0, 0, 1.0, 2.0], [0, 0, 0, 0.0, 1.0]], F)
    stop = np.array([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, np.inf, 3.0], F)
    assert OC.np_stop(occ, stop).tolist() == [2.0, 3.0, 3.0, 3.0, 2.0, 3.0, 3.0, 2.0, 3.0]


# ---------------------------------------------------------------------------------------- ops.ray_parameter
def test_ray_parameter_puts_the_point_at_the_camera_space_depth():
    K, T = syn.camera(S.H, S.W, S.ORBIT)
    rays = O.generate_rays(K, T, S.H, S.W)
    zcam = torch.linspace(2.0, 9.0, rays.shape[0])
    t = ops.ray_parameter(rays, T, zcam)
    assert t.shape == (rays.shape[0],) and t.dtype == torch.float32
    T64 = torch.as_tensor(T, dtype=torch.float64)
    point = rays[:, 0:3].double() + t.double().unsqueeze(1) * rays[:, 3:6].double()
    cam = (point - T64[:3, 3]) @ T64[:3, :3]              # R^T (p - c), row-wise
    assert float((cam[:, 2] - zcam.double()).abs().max()) <= 1e-5
    assert bool((t >= zcam - 1e-5).all()) and float((t - zcam).max()) > 1e-3      # (off-axis rays travel further)
    assert float((ops.ray_parameter(rays, T, 4.0) - ops.ray_parameter(rays, T, torch.full((rays.shape[0],), 4.0))).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------- the Python refusals
def _model():
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    return build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=2)), camera_num=1)


def test_render_rays_occluded_refusals(monkeypatch):
    from stnerf_amd import parallel
    model, rays, occ = _model(), torch.zeros(4, 9), torch.zeros(4, 5)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.render_rays_occluded(rays, occ)
    model.eval()
    with torch.no_grad():
        with pytest.raises(ValueError, match="stops=True.*without early ray termination"):
            model.render_rays_occluded(rays, occ, stops=True)
        with pytest.raises(ValueError, match=r"\(4,5\)"):
            model.render_rays_occluded(rays, torch.zeros(4, 4))
        with pytest.raises(ValueError, match=r"\(4,5\)"):
            model.render_rays_occluded(rays, torch.zeros(5, 5))
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.render_rays_occluded(rays, occ)           # (eval mode, one rank: on to the render path, which has no CPU form)
        model.set_termination(1e-4)
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.render_rays_occluded(rays, occ, stops=True)
        model.set_termination(None)
        monkeypatch.setattr(parallel.dist, "is_initialized", lambda: True)
        monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 2)
        monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 0)
        model.shard_views = True
        with pytest.raises(RuntimeError, match="more than one rank"):
            model.render_rays_occluded(rays, occ)
        K, T = syn.camera(64, 64, 15.0)
        with pytest.raises(RuntimeError, match="more than one rank"):
            parallel.render_view(model, K, T, 64, 64, [1.0, 1.0, 1.0], chuncks=512, device="cpu", occluder=torch.zeros(64 * 64, 5))


def test_render_pose_refuses_an_occluder_of_another_shape():
    from stnerf_amd.render.render_pose import render_pose
    K, T = syn.camera(4, 6, 15.0)
    for rgba, depth in ((torch.zeros(4, 6, 3), torch.zeros(4, 6)), (torch.zeros(4, 6, 4), torch.zeros(4, 6, 1)),
                        (torch.zeros(6, 4, 4), torch.zeros(6, 4))):
        with pytest.raises(ValueError, match="occluder must be"):
            render_pose(_model(), T, K, 4, 6, [(0, 1.0)], 20.0, occluder=(rgba, depth))


def test_ops_check_shapes_and_refuse_cpu_tensors():
    t, raw, w = torch.zeros(4, 3, 8), torch.zeros(4, 3, 8, 4), torch.zeros(4, 3, 8)
    scene, mixed, occ = torch.zeros(4, 3, 5), torch.zeros(4, 5), torch.zeros(4, 5)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.scene_occluder(t, raw, None, w, scene, mixed, occ)
    with pytest.raises(ValueError, match="scene_occluder"):
        ops.scene_occluder(t, raw, None, w, scene, mixed, torch.zeros(4, 4))
    with pytest.raises(ValueError, match="scene_occluder"):
        ops.scene_occluder(t, raw, None, torch.zeros(4, 3, 7), scene, mixed, occ)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.occluder_stop(occ, torch.zeros(4))
    with pytest.raises(ValueError, match="occluder_stop"):
        ops.occluder_stop(occ, torch.zeros(5))
    nets, params = hip.Nets(), hip.RenderParams()
    params.l, params.n1, params.n2, params.ray_stride = 3, 8, 4, 9
    rays, boxes, ws = torch.zeros(4, 9), torch.zeros(3, 8, 3), torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs scene=True"):
        ops.render_rays(rays, boxes, nets, params, ws, occluder=occ)
    with pytest.raises(ValueError, match=r"\(4,5\)"):
        ops.render_rays(rays, boxes, nets, params, ws, scene=True, occluder=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="occluder_stops without an occluder"):
        ops.render_rays(rays, boxes, nets, params, ws, scene=True, occluder_stops=True)
    assert ops.PROFILE_KERNELS[14:16] == ("scene_occluder", "occluder_stop") and ops.PROFILE_KERNELS[13] == "copy_layer_raw_listed"


# ---------------------------------------------------------------------------------------- header, prototypes, library
_CTYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "void*": C.c_void_p,
           "int32_t*": C.c_void_p, "int64_t*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "int32_t": C.c_int32, "float": C.c_float,
           "stnerf_stream_t": C.c_void_p, "const int32_t*": C.POINTER(C.c_int32), "const stnerf_composite_params*": C.POINTER(hip.CompositeParams),
           "const stnerf_nets*": C.POINTER(hip.Nets), "const stnerf_render_params*": C.POINTER(hip.RenderParams),
           "const stnerf_bkgd_cache*": C.POINTER(hip.BkgdCache), "const stnerf_layer_rotation*": C.POINTER(hip.LayerRotation),
           "const stnerf_occupancy*": C.POINTER(hip.Occupancy), "const stnerf_layer_cache*": C.POINTER(hip.LayerCache)}


def _declared(name):
    """[(C type, argument name)] of the header's declaration of ``name``."""
    decl = HEADER[HEADER.index("int " + name + "("):]
    args = decl[decl.index("(") + 1:decl.index(");")]
    out = []
    for a in args.split(","):
        ctype, arg = re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", a).groups()
        out.append((ctype.replace(" *", "*"), arg))
    return out


def test_prototypes_agree_with_the_header():
    for name in NEW:
        assert len(re.findall(r"^int " + name + r"\(", HEADER, re.M)) == 1, name
        assert name in hip.exported_symbols()
        res, args = hip._PROTOS[name]
        declared = _declared(name)
        assert res is C.c_int and len(args) == len(declared), (name, len(args), len(declared))
        for k, ((ctype, arg), got) in enumerate(zip(declared, args)):
            want = _CTYPES[ctype]
            if ctype == "const float*" and arg == "layer_alpha_host":     # (a host table: the one float pointer ctypes fills itself)
                want = C.POINTER(C.c_float)
            assert got is want or got == want, (name, k, ctype, arg, got)
    # the newest sibling is the old entry plus five arguments, in this order, in front of the stream
    old, new = _declared("stnerf_render_rays_layers"), _declared("stnerf_render_rays_occluded")
    assert new[:len(old) - 1] == old[:-1] and new[-1] == old[-1]
    assert [a for _, a in new[len(old) - 1:-1]] == ["occluder", "occluder_stops", "occluded_mixed", "occluded_scene", "occluder_share"]
    assert [a for _, a in _declared("stnerf_scene_occluder")] == [
        "t", "raw", "mask", "merged_weights", "n", "l", "S", "params_host", "scene_in", "mixed_in", "occluder", "occluded_mixed",
        "occluded_scene", "occluder_share", "front_out", "behind_out", "stream"]
    assert [a for _, a in _declared("stnerf_occluder_stop")] == ["occluder", "n", "t_stop", "stream"]
    # no existing entry changed shape
    assert len(_declared("stnerf_render_rays_layers")) == 31 and len(_declared("stnerf_composite_scene")) == 15


def test_library_checks_arguments_before_any_launch():
    lib = hip.lib()
    null, fake = C.c_void_p(0), 1 << 20
    p = ops.composite_params()
    ok = [fake, fake, null, fake, 8, 3, 64, C.byref(p), fake, fake, fake, fake, null, null, null, null, null]
    call = lambda over: lib.stnerf_scene_occluder(*[over.get(i, v) for i, v in enumerate(ok)])     # {argument index: value}
    assert call({4: 0}) == hip.OK                         # n = 0: nothing to launch
    for i in (0, 1, 3, 8, 9, 10):                                    # t, raw, merged_weights, scene_in, mixed_in, occluder
        assert call({i: null}) == hip.EINVAL and "null pointer" in hip.last_error(), i
    assert call({7: None}) == hip.EINVAL and "null pointer" in hip.last_error()
    assert call({11: null}) == hip.EINVAL and "occluded_mixed is required" in hip.last_error()
    for l, s in ((0, 64), (17, 64), (3, 0), (16, 4096)):
        assert call({5: l, 6: s}) == hip.EINVAL, (l, s)
    assert "65535" in hip.last_error()
    assert call({4: -1}) == hip.EINVAL
    assert call({1: fake + 8}) == hip.EINVAL and "16-byte aligned" in hip.last_error()
    assert lib.stnerf_occluder_stop(null, 4, fake, null) == hip.EINVAL and lib.stnerf_occluder_stop(fake, 4, null, null) == hip.EINVAL
    assert lib.stnerf_occluder_stop(fake, 0, fake, null) == hip.OK
    # the pipeline entry: an occluder without the scene passes or without occluded_mixed; the outputs or the stop without an occluder
    nets, rp = hip.Nets(), hip.RenderParams()
    rp.l, rp.n1, rp.n2, rp.ray_stride = 3, 8, 4, 9
    nets.bkgd = nets.bkgd_fine = fake
    base = [fake, 4, fake, 0, C.byref(nets), C.byref(rp), null, null, fake, 1 << 30, fake, fake, fake, fake, fake, None, None]
    tail = lambda scene, flags, occ, stops, om: [scene, None, None, null, None, null, 0.0, flags, null, None, null, None, null,
                                                 occ, stops, om, null, null, null]
    run = lambda *a: lib.stnerf_render_rays_occluded(*(base + tail(*a)))
    assert run(null, None, fake, 0, fake) == hip.EINVAL and "needs scene_out and occluded_mixed" in hip.last_error()
    assert run(fake, None, fake, 0, null) == hip.EINVAL and "needs scene_out and occluded_mixed" in hip.last_error()
    assert run(fake, None, null, 1, null) == hip.EINVAL and "without an occluder" in hip.last_error()
    assert run(fake, None, null, 0, fake) == hip.EINVAL and "without an occluder" in hip.last_error()
    assert run(fake, None, fake, 1, fake) == hip.EINVAL and "occluder_stops needs early ray termination" in hip.last_error()
    flags = (C.c_int32 * 3)(0, 0, 0)
    assert run(fake, flags, fake, 1, fake) == hip.EINVAL and "occluder_stops needs early ray termination" in hip.last_error()
    # the workspace is the one stnerf_render_rays_layers needs: no query of its own, no argument of the old queries changed
    assert not any("workspace_bytes_occlu" in s for s in hip.exported_symbols())


# ---------------------------------------------------------------------------------------- the renderer's bookkeeping
@pytest.mark.parametrize("walking", [False, True])
def test_renderer_occluder_bookkeeping(monkeypatch, walking):
    """Against a stub model and a stub ``render_pose``: the callable is asked once per frame, a frame it returns None for renders
    as ever, the others keep ``images_occluded`` and hand ``on_frame`` the keyword ``occluded``; ``scene=`` only with ``scene_passes``."""
    from stnerf_amd.render import layered_neural_renderer as lnr
    from test_scene_passes_cpu import StubModel
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[6, 4]))
    K, T = syn.camera(4, 6, 15.0)
    calls = []

    def fake_render_pose(model_, pose, K_, h, w, pairs, far, thr=0, bthr=0, device="cuda", scene_passes=False, occluder=None, occluder_stops=False):
        calls.append((scene_passes, occluder is not None, occluder_stops))
        g = torch.Generator().manual_seed(len(calls))
        images = lambda c, k=3: [torch.rand(h, w, c, generator=g) for _ in range(k)]
        color, depth = images(3, 1)[0], images(1, 1)[0]
        if not scene_passes and occluder is None:
            return color, depth, images(3), images(1)
        passes = dict(color_scene=images(3), alpha_scene=images(1), depth_scene=images(1))
        if occluder is not None:
            assert tuple(occluder[0].shape) == (h, w, 4) and tuple(occluder[1].shape) == (h, w)
            passes.update(color_occluded=images(3, 1)[0], alpha_occluded=images(1, 1)[0], depth_occluded=images(1, 1)[0],
                          color_scene_occluded=images(3), alpha_scene_occluded=images(1), depth_scene_occluded=images(1),
                          occluder_share=tuple(images(3, 1) + images(1, 2)))
        return color, depth, images(3), images(1), passes

    monkeypatch.setattr(lnr, "_render_pose", fake_render_pose)
    asked = []

    def card(idx, pose, K_):
        asked.append(idx)
        return None if idx == 1 else (torch.zeros(4, 6, 4), torch.ones(4, 6))
    r = lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], occluder=card, occluder_stops=True)
    r.set_path_fixed_gt_poses(0, 3)
    seen = []
    (r.render_path_walking if walking else r.render_path)(inverse_y_axis=True, on_frame=lambda idx, c, d, cl, dl, occluded: seen.append((idx, occluded)))
    assert asked == [0, 1, 2] and calls == [(True, True, True), (False, False, False), (True, True, True)]
    assert [o is None for _, o in seen] == [False, True, False] and len(r.images_occluded) == 2
    keys = ["alpha_occluded", "alpha_scene_occluded", "color_occluded", "color_scene_occluded", "depth_occluded", "depth_scene_occluded", "occluder_share"]
    assert sorted(seen[0][1]) == keys and isinstance(seen[0][1]["occluder_share"], tuple) and len(seen[0][1]["color_scene_occluded"]) == 3
    assert torch.equal(r.images_occluded[0], seen[0][1]["color_occluded"]) and torch.equal(r.images_occluded[1], seen[2][1]["color_occluded"])
    assert all(len(x) == 0 for x in r.images_scene)              # (the plain passes are kept only with scene_passes)
    with pytest.raises(TypeError, match="callable"):
        lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], occluder=(torch.zeros(4, 6, 4), torch.ones(4, 6)))
    # without an occluder the five-argument callback and the lists are what they were
    r0 = lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K])
    r0.set_path_fixed_gt_poses(0, 3)
    (r0.render_path_walking if walking else r0.render_path)(on_frame=lambda idx, c, d, cl, dl: None)
    assert r0.images_occluded == [] and r0.occluder is None
