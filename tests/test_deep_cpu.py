"""Deep frames without a GPU (include/stnerf.h / DESIGN.md sections 4.2 and 7): the numpy restatement of tests/deep_common.py
against hand-worked rays (the kept rule at w == w_min, a NaN weight, a NaN depth, bins at an exact multiple of merge_dz, a ray with
nothing kept, element ties in z, absent rows); on the oracle, a deep frame built from what ``O.render_chunk`` traces, with one
element against ``occluder_common``'s oracle statement and with two against a hand-written two-step over; the Python refusals; and
that the header, the prototypes and the library agree on the new entries."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import stnerf_oracle as O
from stnerf_amd import hip, ops, synthetic as syn
from stnerf_amd.deep import DeepFrame, DeepSpec, piece_rays

import deep_common as DC
import occluder_common as OCL
import scene_edits_common as S

HEADER = open(os.path.join(REPO, "include", "stnerf.h")).read()
NEW = ("stnerf_deep_workspace_bytes", "stnerf_deep_count", "stnerf_deep_offsets", "stnerf_deep_fill", "stnerf_deep_composite")
F = np.float32


def one_ray(t, w, colour=None, have=True):
    t, w = np.asarray(t, F).reshape(1, 1, -1), np.asarray(w, F).reshape(1, 1, -1)
    colour = np.ones(t.shape + (3,), F) if colour is None else np.asarray(colour, F).reshape(t.shape + (3,))
    return t, w, colour, np.array([[have]])


# ---------------------------------------------------------------------------------------- the restatement, by hand
def test_the_kept_rule_at_w_min_a_nan_weight_and_a_layer_without_output():
    t, w, c, have = one_ray([1, 2, 3, 4, 5], [0.25, 1e-3, np.nextafter(F(1e-3), F(1)), np.nan, 0.0])
    counts, offsets, rec = DC.np_deep(t, w, c, have, w_min=1e-3)
    layer, first_k, count = DC.meta_of(rec)
    assert counts.tolist() == [3] and offsets.tolist() == [0, 3]
    assert first_k.tolist() == [0, 2, 3] and count.tolist() == [1, 1, 1] and layer.tolist() == [0, 0, 0]      # w == w_min is dropped
    assert rec[0, :7].tolist() == [0.25, 0.25, 0.25, 0.25, 0.25, 1.0, 1.0] and np.isnan(rec[2, 0:5]).all() and rec[2, 5] == 4.0
    assert DC.np_deep(t, w, c, have, w_min=0.0)[0].tolist() == [4]                                            # the exact zero goes
    assert DC.np_deep(t, w, c, ~have)[0].tolist() == [0] and DC.np_deep(t, w, c, ~have)[2].shape == (0, 8)


def test_bins_at_an_exact_multiple_of_merge_dz_and_a_nan_depth():
    # t0 = 1; (t - 1) / 0.25 = 0, 0.5, 1 exactly (a new bin AT the multiple), 1.996, NaN, 2.0, 2.2, back to bin 0
    t, w, c, have = one_ray([1.0, 1.125, 1.25, 1.499, np.nan, 1.5, 1.55, 1.0], [0.125] * 8)
    counts, _, rec = DC.np_deep(t, w, c, have, merge_dz=0.25)
    layer, first_k, count = DC.meta_of(rec)
    assert first_k.tolist() == [0, 2, 4, 5, 7] and count.tolist() == [2, 2, 1, 2, 1] and counts.tolist() == [5]
    assert rec[0, 3] == 0.25 and rec[0, 4] == F(F(0.125) * F(1.0)) + F(F(0.125) * F(1.125)) and rec[0, 5:7].tolist() == [1.0, 1.125]
    assert np.isnan(rec[2, 4:7]).all() and rec[2, 3] == 0.125                      # the NaN depth: a segment of its own
    assert rec[3, 5:7].tolist() == [1.5, F(1.55)]
    # a dropped sample inside a bin does not cut the segment; the count is of kept samples
    t, w, c, have = one_ray([1.0, 1.01, 1.02], [0.5, 0.0, 0.25])
    _, _, rec = DC.np_deep(t, w, c, have, merge_dz=0.25)
    assert DC.meta_of(rec)[2].tolist() == [2] and rec[0, 3] == 0.75 and rec[0, 6] == F(1.02)
    # merge_dz = 0: every kept sample its own record
    assert DC.np_deep(t, w, c, have)[0].tolist() == [2]


def test_layers_are_layer_major_and_a_ray_with_nothing_kept_is_empty():
    t = np.array([[[1, 2], [1, 2]], [[1, 2], [1, 2]], [[3, 4], [0.5, 0.6]]], F)
    w = np.array([[[0.5, 0.25], [0.125, 0]], [[0, 0], [0, 0]], [[0.5, 0], [0.25, 0.25]]], F)
    c = np.ones((3, 2, 2, 3), F)
    counts, offsets, rec = DC.np_deep(t, w, c, np.ones((3, 2), bool))
    assert counts.tolist() == [3, 0, 3] and offsets.tolist() == [0, 3, 3, 6]
    assert DC.meta_of(rec)[0].tolist() == [0, 0, 1, 0, 1, 1] and DC.meta_of(rec)[1].tolist() == [0, 1, 0, 0, 0, 1]
    mixed, scene, shares = DC.np_deep_composite(offsets, rec, 2)
    assert not mixed[1].any() and mixed[0].tolist() == [0.875, 0.875, 0.875, F(0.5 + 0.5 + 0.125), 0.875] and shares.shape == (3, 0, 5)
    assert scene[2, 1].tolist() == [0.5, 0.5, 0.5, F(F(0.25 * 0.5) + F(0.25) * F(0.6)), 0.5]


def test_element_ties_in_z_are_stable_and_absent_rows_change_nothing():
    t, w, c, have = one_ray([1, 2, 3, 4], [0.25, 0.25, 0.25, 0.125])
    _, offsets, rec = DC.np_deep(t, w, c, have)
    row = lambda r, a, z: [r, r, r, a, z]
    # two present rows at z = 3 (tied: index order), absent ones of every kind around them
    el = np.array([[row(0.1, 0.0, 2.0), row(0.5, 0.5, 3.0), row(0.2, np.nan, 1.0), row(1.0, 0.25, 3.0), row(np.nan, 1.0, np.inf),
                    row(np.inf, 1.0, np.nan), row(0.3, -1.0, 1.0), row(0.4, 2.0, -np.inf)]], F)
    ap, z, order = DC.np_rows(el[0])
    assert order[:2].tolist() == [1, 3] and ap.tolist() == [0, 0.5, 0, 0.25, 0, 0, 0, 0] and np.isinf(z[[0, 2, 4, 5, 6, 7]]).all()
    mixed, scene, shares = DC.np_deep_composite(offsets, rec, 1, el)
    two = DC.np_deep_composite(offsets, rec, 1, el[:, [1, 3]])
    assert np.array_equal(mixed, two[0]) and np.array_equal(shares[:, [1, 3]], two[2]) and not shares[:, [0, 2, 4, 5, 6, 7]].any()
    # by hand: in front of z = 3 the weights 0.25 + 0.25, T = 0.5; behind both: q = 0.5 * 0.75
    q = F(0.375)
    assert scene[0, 0, 4] == F(0.25 + 0.25 + q * F(0.25) + q * F(0.125))
    assert shares[0, 1].tolist() == [0.125, 0.125, 0.125, 0.75, 0.25]                         # s = 0.5 * 0.5
    assert shares[0, 3].tolist() == [F(0.0625), F(0.0625), F(0.0625), F(0.0625 * 3), 0.0625]  # s = 0.25 * 0.5 * (1 - 0.5), r = 1
    assert mixed[0, 4] == F(F(scene[0, 0, 4] + F(0.25)) + F(0.0625))
    # the tie the other way round is another stack
    swapped = DC.np_deep_composite(offsets, rec, 1, el[:, [3, 1]])
    assert swapped[2][0, 0, 4] == 0.125 and swapped[2][0, 1, 4] == F(0.5 * 0.5 * 0.75)
    # a sample AT z is behind; a NaN zf is in front
    t, w, c, have = one_ray([3.0, np.nan], [0.5, 0.25])
    _, offsets, rec = DC.np_deep(t, w, c, have)
    _, scene, shares = DC.np_deep_composite(offsets, rec, 1, np.array([[row(1.0, 1.0, 3.0)]], F))
    assert scene[0, 0, 4] == 0.25 and shares[0, 0, 4] == 0.75


def test_the_wave_total_is_the_scan_ladder():
    g = np.random.default_rng(0)
    v = g.standard_normal((5, 64)).astype(F)
    got = DC.np_wave_total(v)
    rows = []
    for r in range(4):                                              # a row of 16: the Hillis-Steele ladder, then the rows in order
        x = v[:, 16 * r:16 * r + 16].copy()
        for d in (1, 2, 4, 8):
            y = x.copy()
            y[:, d:] = x[:, :-d] + x[:, d:]
            x = y
        rows.append(x[:, 15])
    want = (rows[0] + rows[1]) + ((rows[2] + rows[3]))
    assert np.array_equal(got, ((rows[0] + rows[1]).astype(F) + (rows[2] + rows[3]).astype(F)).astype(F)) and want.dtype == F
    assert np.allclose(got, v.astype(np.float64).sum(1), rtol=0, atol=64 * 2.0 ** -24 * np.abs(v).sum(1).max())


# ---------------------------------------------------------------------------------------- on the oracle
@pytest.fixture(scope="module")
def traced():
    """The oracle case chunk by chunk, as ``occluder_common.oracle_occluded`` runs it -> fp32 numpy t, wm (N,l,S), colour
    (N,l,S,3), scene (N,l,5), mixed (N,5), and the deep list of the restatement at w_min = 0, merge_dz = 0."""
    case = OCL.oracle_case()
    rays, m = S.case_rays(case), S.oracle_model(case, torch.float32)
    jitter, u = S.case_draws(case)
    l, step, n = S.total_layers(case), case["chunk"], rays.shape[0]
    parts = {k: [] for k in ("t", "wm", "colour", "scene", "mixed")}
    with torch.no_grad():
        for s in range(0, n, step):
            e = min(s + step, n)
            draws = iter([jitter[i, s:e] for i in range(l)] + [u[i, s:e] for i in range(l)])
            trace = {}
            out = O.render_chunk(m, rays[s:e].float(), rand=lambda shape: next(draws), trace=trace, scene=True,
                                 density_threshold=case["thr"], bkgd_density_threshold=case["bthr"])
            parts["t"].append(torch.stack(trace["t_fine"], 1))
            parts["colour"].append(torch.stack([torch.sigmoid(c) for c in trace["rgb_fine"]], 1))
            parts["wm"].append(trace["merged_weights"])
            parts["scene"].append(torch.stack([torch.cat(p, -1) for p in out[5]], 1))
            parts["mixed"].append(torch.cat(out[0], -1))
    d = {k: torch.cat(v, 0) for k, v in parts.items()}
    t, wm, colour = (d[k].numpy().astype(F) for k in ("t", "wm", "colour"))
    _, offsets, rec = DC.np_deep(t, wm, colour, np.ones(t.shape[:2], bool))
    return dict(d, l=l, offsets=offsets, rec=rec, np_t=t, np_wm=wm, np_colour=colour)


def sums_bound(traced):
    """gamma(l S) sum |wM x| per ray and channel: two fp32 sums of the ray's l S products in different orders differ by twice it."""
    x = np.concatenate([traced["np_colour"], traced["np_t"][..., None], np.ones_like(traced["np_t"])[..., None]], -1).astype(np.float64)
    wx = np.abs(traced["np_wm"].astype(np.float64)[..., None] * x)
    l, S_ = traced["np_t"].shape[1:]
    return DC.gamma(l * S_) * wx.sum((1, 2)), wx


def test_flatten_of_the_oracles_deep_frame_is_its_mixed_image(traced):
    mixed, scene, _ = DC.np_deep_composite(traced["offsets"], traced["rec"], traced["l"])
    bound, _ = sums_bound(traced)
    assert int(traced["offsets"][-1]) > 4 * S.N
    assert (np.abs(mixed.astype(np.float64) - traced["mixed"].numpy()) <= 2 * bound).all()
    assert (np.abs(scene.astype(np.float64) - traced["scene"].numpy()) <= 2 * bound[:, None, :]).all()


def test_one_element_is_the_occluder_statement_of_the_oracle(traced):
    occ = OCL.case_occluder()
    ref = OCL.torch_occluded(traced["t"], traced["colour"], traced["wm"], traced["scene"], traced["mixed"], torch.from_numpy(occ))
    mixed, scene, shares = DC.np_deep_composite(traced["offsets"], traced["rec"], traced["l"], occ[:, None, :])
    present = ref["present"].numpy()
    bound, wx = sums_bound(traced)
    rows = np.abs(np.concatenate([occ[:, 0:3], occ[:, 4:5], np.ones((S.N, 1), F)], 1)).astype(np.float64)
    share_bound = (2 * DC.gamma(wx.shape[1] * wx.shape[2]) * wx[..., 4].sum((1, 2)) + 6 * DC.U)[:, None] * rows
    assert int(present.sum()) > 200
    assert (np.abs(shares[:, 0].astype(np.float64) - ref["share"].numpy())[present] <= share_bound[present]).all()
    assert (np.abs(scene.astype(np.float64) - ref["scene"].numpy())[present] <= 2 * bound[present][:, None, :] + 2 * DC.U).all()
    assert (np.abs(mixed.astype(np.float64) - ref["mixed"].numpy())[present] <= (2 * bound + share_bound + 8 * DC.U * (1 + rows))[present]).all()
    # an absent row: the flatten, and no share
    flat = DC.np_deep_composite(traced["offsets"], traced["rec"], traced["l"])[0]
    assert np.array_equal(mixed[~present], flat[~present]) and not shares[~present].any()
    # the occluder shows
    assert int((np.abs(mixed - flat).max(1)[present] > 1e-2).sum()) >= 100


def test_two_elements_are_a_two_step_over(traced):
    """A half-transparent prop at z1 and an opaque card behind it at z2 > z1, written out: a sample in front of z1 keeps its weight,
    one between loses (1 - a1), one behind z2 loses (1 - a1)(1 - a2); each element takes a' times what is left in front of it."""
    n = S.N
    occ = OCL.case_occluder()
    el = np.zeros((n, 2, 5), F)
    el[:, 1] = [0.9, 0.1, 0.2, 0.5, 0.0]                            # listed second, nearer: the sort matters
    el[:, 1, 4] = occ[:, 4]
    el[:, 0] = [0.2, 0.8, 0.4, 1.0, 0.0]
    el[:, 0, 4] = occ[:, 4] + F(1.5)
    mixed, scene, shares = DC.np_deep_composite(traced["offsets"], traced["rec"], traced["l"], el)
    t, wm = traced["np_t"].astype(np.float64), traced["np_wm"].astype(np.float64)
    x = np.concatenate([traced["np_colour"].astype(np.float64), t[..., None], np.ones_like(t)[..., None]], -1)
    z1, z2 = el[:, 1, 4].astype(np.float64)[:, None, None], el[:, 0, 4].astype(np.float64)[:, None, None]
    a1, a2 = 0.5, 1.0
    b1, b2 = traced["np_t"] >= el[:, 1, 4][:, None, None], traced["np_t"] >= el[:, 0, 4][:, None, None]
    q = np.where(b2, (1 - a1) * (1 - a2), np.where(b1, 1 - a1, 1.0))
    passes = (q[..., None] * wm[..., None] * x).sum(2)
    T1 = np.clip(1 - np.where(b1, 0, wm).sum((1, 2)), 0, None)
    T2 = np.clip(1 - np.where(b2, 0, wm).sum((1, 2)), 0, None)
    row = lambda e: np.concatenate([el[:, e, 0:3], el[:, e, 4:5], np.ones((n, 1), F)], 1).astype(np.float64)
    s1, s2 = (a1 * T1)[:, None] * row(1), (a2 * T2 * (1 - a1))[:, None] * row(0)
    want = passes.sum(1) + s1 + s2
    bound, wx = sums_bound(traced)
    share_bound = (2 * DC.gamma(wx.shape[1] * wx.shape[2]) * wx[..., 4].sum((1, 2)) + 8 * DC.U)[:, None]
    assert (np.abs(shares[:, 1] - s1) <= share_bound * np.abs(row(1))).all() and (np.abs(shares[:, 0] - s2) <= share_bound * np.abs(row(0))).all()
    assert (np.abs(scene - passes) <= 2 * bound[:, None, :] + 4 * DC.U).all()
    assert (np.abs(mixed - want) <= 2 * bound + share_bound * (np.abs(row(0)) + np.abs(row(1))) + 16 * DC.U * (1 + np.abs(want))).all()
    assert int((np.abs(shares[:, 0, 4]) > 1e-3).sum()) >= 50 and int((np.abs(shares[:, 1, 4]) > 1e-3).sum()) >= 100


# ---------------------------------------------------------------------------------------- the Python layer
def _model():
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    return build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=2)), camera_num=1)


def test_the_spec_and_the_package_names():
    import stnerf_amd
    assert stnerf_amd.DeepSpec is DeepSpec and stnerf_amd.DeepFrame is DeepFrame
    assert DeepSpec() == DeepSpec(0.0, 0.0) and DeepSpec(1e-3, 0.25).options(7) == dict(w_min=1e-3, merge_dz=0.25, capacity=7)
    for bad in (dict(w_min=-1.0), dict(w_min=float("nan")), dict(merge_dz=-0.1), dict(merge_dz=float("inf"))):
        with pytest.raises(ValueError, match="finite and >= 0"):
            DeepSpec(**bad)
    assert piece_rays(4, 192) == (1 << 30) // (32 * 4 * 192) and piece_rays(16, 256, budget=1) == 1


def test_render_rays_deep_refusals(monkeypatch):
    from stnerf_amd import parallel
    from stnerf_amd.render.render_pose import render_pose
    model, rays = _model(), torch.zeros(4, 9)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.render_rays_deep(rays)
    model.eval()
    K, T = syn.camera(4, 6, 15.0)
    with torch.no_grad():
        with pytest.raises(TypeError, match="DeepSpec"):
            model.render_rays_deep(rays, dict(w_min=0.0))
        with pytest.raises(ValueError, match=r"\(4,5\)"):
            model.render_rays_deep(rays, occluder=torch.zeros(4, 4))
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            model.render_rays_deep(rays, DeepSpec())
        for name, value in (("accumulate", dict(passes=2)), ("lattice", dict()), ("reproject", (dict(), []))):
            with pytest.raises(ValueError, match=f"deep=.*{name}=.*not one sample list per pixel"):
                render_pose(model, T, K, 4, 6, [(0, 1.0)], 20.0, deep=DeepSpec(), **{name: value})
        with pytest.raises(ValueError, match="occluder_stops"):
            parallel.render_view(model, K, T, 4, 6, [1.0, 1.0, 1.0], device="cpu", deep=DeepSpec(), occluder=torch.zeros(24, 5), occluder_stops=True)
        monkeypatch.setattr(parallel.dist, "is_initialized", lambda: True)
        monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 2)
        monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 0)
        model.shard_views = True
        with pytest.raises(RuntimeError, match="more than one rank"):
            model.render_rays_deep(rays)
        K, T = syn.camera(64, 64, 15.0)
        with pytest.raises(RuntimeError, match="more than one rank"):
            parallel.render_view(model, K, T, 64, 64, [1.0, 1.0, 1.0], chuncks=512, device="cpu", deep=DeepSpec())


def test_ops_check_shapes_and_refuse_cpu_tensors():
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="alike"):
        ops.deep_count(z(2, 3, 4), None, z(2, 3, 5))
    with pytest.raises(ValueError, match="mask must be"):
        ops.deep_count(z(2, 3, 4), torch.zeros(2, 4, dtype=torch.uint8), z(2, 3, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.deep_count(z(2, 3, 4), None, z(2, 3, 4))
    with pytest.raises(ValueError, match="samples \\(capacity,8\\)"):
        ops.deep_fill(z(2, 3, 4), z(2, 3, 4, 4), None, z(2, 3, 4), torch.zeros(3, dtype=torch.int64), z(5, 7))
    with pytest.raises(ValueError, match="rows of"):
        ops.deep_composite(torch.zeros(3, dtype=torch.int64), z(0, 8), 2, z(2, 5))
    with pytest.raises(ValueError, match="scene=True"):
        ops.render_rays(z(4, 9), z(3, 8, 3), hip.Nets(), hip.RenderParams(l=3), torch.zeros(8, dtype=torch.uint8), deep=dict())
    with pytest.raises(ValueError, match="w_min, merge_dz and capacity"):
        ops.render_rays(z(4, 9), z(3, 8, 3), hip.Nets(), hip.RenderParams(l=3), torch.zeros(8, dtype=torch.uint8), scene=True, deep=dict(dz=1))
    with pytest.raises(ValueError, match="DeepFrame"):
        DeepFrame(torch.zeros(5, dtype=torch.int64), z(0, 8), 2, 3, 2)


def test_frame_bookkeeping_without_a_gpu(tmp_path):
    """from_pieces rebases the offsets; stats, meta and the npz round trip are plain host code."""
    rec = np.zeros((5, 8), F)
    rec.view(np.uint32)[:, 7] = [0 | 1 << 8 | 1 << 16, 1 | 2 << 8 | 3 << 16, 0, 2 | 255 << 8 | 2 << 16, 1]
    rec[3, 0] = np.nan
    a = (torch.tensor([0, 2, 2]), torch.from_numpy(rec[:2].copy()))
    b = (torch.tensor([0, 0, 3]), torch.from_numpy(rec[2:].copy()))
    frame = DeepFrame.from_pieces([a, b], 2, 2, 3, far=20.0)
    assert frame.offsets.tolist() == [0, 2, 2, 2, 5] and frame.samples.shape == (5, 8) and frame.n_pixels == 4
    layer, first_k, count = frame.meta()
    assert layer.tolist() == [0, 1, 0, 2, 1] and first_k.tolist() == [1, 2, 0, 255, 0] and count.tolist() == [1, 3, 0, 2, 0]
    st = frame.stats()
    assert st == dict(pixels=4, samples=5, mean=1.25, max=3, histogram=[2, 0, 1, 1], bytes=5 * 32 + 5 * 8)
    path = str(tmp_path / "f.npz")
    frame.save(path)
    back = DeepFrame.load(path)
    assert torch.equal(back.offsets, frame.offsets) and torch.equal(back.samples.view(torch.int32), frame.samples.view(torch.int32))
    assert (back.H, back.W, back.layers, back.far) == (2, 2, 3, 20.0)


def test_no_piece_is_the_empty_frame():
    frame = DeepFrame.from_pieces([], 1, 0, 3)
    assert frame.offsets.tolist() == [0] and frame.samples.shape == (0, 8) and frame.n_pixels == 0
    assert frame.stats() == dict(pixels=0, samples=0, mean=0.0, max=0, histogram=[0], bytes=8)


@pytest.mark.parametrize("walking", [False, True])
def test_renderer_deep_bookkeeping_and_refusals(monkeypatch, walking):
    """Against a stub model and a stub ``render_pose``: every frame is rendered with ``deep=`` the spec, its frame is kept in
    ``deep_frames`` (unflipped: a list has no rows to flip) and handed to ``on_frame`` as ``deep=``; ``scene=`` only with
    ``scene_passes``; the constructor refuses accumulate, lattice, reproject and occluder_stops."""
    from stnerf_amd.render import layered_neural_renderer as lnr
    from test_scene_passes_cpu import StubModel
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[6, 4]))
    K, T = syn.camera(4, 6, 15.0)
    calls, made = [], []

    def fake_render_pose(model_, pose, K_, h, w, pairs, far, thr=0, bthr=0, device="cuda", scene_passes=False, occluder=None, occluder_stops=False,
                         deep=None):
        calls.append((scene_passes, occluder is not None, deep))
        g = torch.Generator().manual_seed(len(calls))
        images = lambda c, k=3: [torch.rand(h, w, c, generator=g) for _ in range(k)]
        if not scene_passes and deep is None:
            return images(3, 1)[0], images(1, 1)[0], images(3), images(1)
        passes = dict(color_scene=images(3), alpha_scene=images(1), depth_scene=images(1))
        if deep is not None:
            made.append(DeepFrame(torch.zeros(h * w + 1, dtype=torch.int64), torch.zeros(0, 8), h, w, 3, far))
            passes["deep"] = made[-1]
        return images(3, 1)[0], images(1, 1)[0], images(3), images(1), passes

    monkeypatch.setattr(lnr, "_render_pose", fake_render_pose)
    spec = DeepSpec(1e-4, 0.5)
    r = lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], deep=spec)
    r.set_path_fixed_gt_poses(0, 3)
    seen = []
    (r.render_path_walking if walking else r.render_path)(inverse_y_axis=True, on_frame=lambda idx, c, d, cl, dl, deep: seen.append((idx, deep)))
    assert calls == [(True, False, spec)] * 3 and [i for i, _ in seen] == [0, 1, 2]
    assert all(a is b for (_, a), b in zip(seen, made)) and all(a is b for a, b in zip(r.deep_frames, made)) and len(r.deep_frames) == 3
    assert all(len(x) == 0 for x in r.images_scene)              # (the plain passes are kept only with scene_passes)
    assert lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], deep=True).deep == DeepSpec()
    for name, value in (("accumulate", dict(max_spp=2)), ("lattice", dict(levels=1, tol_rgb=0.01)), ("reproject", dict())):
        with pytest.raises(ValueError, match=f"deep= with {name}="):
            lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], deep=spec, **{name: value})
    with pytest.raises(ValueError, match="deep= with occluder_stops"):
        lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], deep=spec, occluder=lambda i, p, k: None, occluder_stops=True)
    with pytest.raises(TypeError, match="DeepSpec"):
        lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K], deep=dict(w_min=0.0))
    # without deep= the five-argument callback and the list are what they were
    r0 = lnr.LayeredNeuralRenderer(cfg, model=StubModel(), gt_poses=T[None], gt_Ks=[K])
    r0.set_path_fixed_gt_poses(0, 3)
    (r0.render_path_walking if walking else r0.render_path)(on_frame=lambda idx, c, d, cl, dl: None)
    assert r0.deep_frames == [] and r0.deep is None and calls[-1] == (False, False, None)


# ---------------------------------------------------------------------------------------- header, prototypes, library
def test_the_new_entries_are_declared_exported_and_check_their_arguments():
    lib = hip.lib()
    for name in NEW:
        assert name in hip.exported_symbols() and getattr(lib, name) is not None and name + "(" in HEADER
    assert ops.PROFILE_KERNELS[16:20] == ("deep_count", "deep_offsets", "deep_fill", "deep_composite") and ops.PROFILE_KERNELS[15] == "occluder_stop"
    assert hip.DEEP_MAX_ELEMENTS == 8 and "#define STNERF_DEEP_MAX_ELEMENTS 8" in HEADER
    assert lib.stnerf_deep_workspace_bytes(0) == 256 and lib.stnerf_deep_workspace_bytes(257) == 512 and lib.stnerf_deep_workspace_bytes(-1) == hip.EINVAL
    assert ops.deep_workspace_bytes(1 << 20) == (1 << 20) // 256 * 4 + 256
    p, null, one = ops.composite_params(), C.c_void_p(0), C.c_void_p(16)
    count = lambda **k: lib.stnerf_deep_count(*[{**dict(t=one, mask=null, wm=one, n=0, l=2, S=8, p=C.byref(p), w_min=0.0, dz=0.0, counts=one, stream=null), **k}[a]
                                                for a in ("t", "mask", "wm", "n", "l", "S", "p", "w_min", "dz", "counts", "stream")])
    assert count() == hip.OK                                           # n == 0: nothing is launched
    for bad in (dict(t=null), dict(wm=null), dict(counts=null), dict(l=0), dict(l=17), dict(S=0), dict(S=257), dict(n=-1),
                dict(w_min=-1e-9), dict(w_min=float("nan")), dict(dz=-1.0), dict(dz=float("nan"))):
        assert count(**bad) == hip.EINVAL, bad
    assert "negative or NaN" in hip.last_error()
    assert lib.stnerf_deep_composite(one, null, 0, 2, null, 0, one, null, null, null) == hip.OK
    assert lib.stnerf_deep_composite(one, null, 0, 2, null, 9, one, null, null, null) == hip.EINVAL and "E = 9" in hip.last_error()
    assert lib.stnerf_deep_composite(one, null, 0, 2, null, 1, one, null, null, null) == hip.EINVAL        # rows missing
    assert lib.stnerf_deep_composite(one, C.c_void_p(8), 0, 2, null, 0, one, null, null, null) == hip.EINVAL and "16-byte" in hip.last_error()
    assert lib.stnerf_deep_offsets(one, 1 << 20, 1 << 12, one, one, 1 << 30, null) == hip.EINVAL and "2^31" in hip.last_error()


def test_both_record_sizes_are_accepted_and_an_all_zero_deep_record_is_no_feature():
    lib = hip.lib()
    base, deep = hip.RenderOptions(), hip.RenderOptionsDeep()
    assert C.sizeof(hip.RenderOptionsDeep) == C.sizeof(hip.RenderOptions) + 48 and deep.struct_size == C.sizeof(hip.RenderOptionsDeep)
    names = [f for f, _ in hip.RenderOptionsDeep._fields_]
    assert names[:len(hip.RenderOptions._fields_)] == [f for f, _ in hip.RenderOptions._fields_]
    assert names[-7:] == ["deep_w_min", "deep_merge_dz", "deep_offsets", "deep_samples", "deep_capacity", "deep_total", "deep_workspace"]
    for n, l, n1, n2 in ((1, 1, 3, 0), (1000, 4, 64, 128), (4096, 3, 12, 6)):
        plain = lib.stnerf_render_workspace_bytes(n, l, n1, n2, 0)
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, 0, C.byref(base)) == plain
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, 0, deep.ref()) == plain
        live = hip.RenderOptionsDeep(deep_samples=16, deep_capacity=1 << 20, deep_offsets=16, deep_total=16, deep_workspace=16)
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, 0, live.ref()) == plain          # the render workspace is unchanged
    deep.struct_size = C.sizeof(hip.RenderOptionsDeep) - 8
    assert lib.stnerf_render_workspace_bytes_opts(1, 1, 3, 0, 0, deep.ref()) == hip.EINVAL and "struct_size" in hip.last_error()


def test_the_c_header_lays_the_deep_record_out_as_ctypes_does(tmp_path):
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    fields = [f for f, _ in hip.RenderOptionsDeep._fields_[len(hip.RenderOptions._fields_):]]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(stnerf_render_options_deep));', 'printf("base %zu\\n", offsetof(stnerf_render_options_deep, base));']
    lines += [f'printf("{f} %zu\\n", offsetof(stnerf_render_options_deep, {f}));' for f in fields] + ['return 0;}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(hip.RenderOptionsDeep) and int(got["base"]) == 0
    for f in fields:
        assert int(got[f]) == getattr(hip.RenderOptionsDeep, f).offset, f
