"""Reprojection of the background across nearby views on the MI355X (csrc/reproject.hip): splat, resolve and
the hole list against the numpy restatement of tests/reproject_common.py, bit for bit, on the case set whose census
tests/test_reproject_cpu.py asserts; then the drivers (``parallel.render_view_reprojected``, ``render_pose(reproject=)`` and the
renderer's ``reproject=``) on the small model of tests/test_gpu_scene_edits_oracle.py and its 17 x 23 view (391 rays), against the
same calls made by hand.

The drivers' scene.  The fixture model's background is a random-weight fog: a quarter of the view's rays composite to alpha
exactly 0 and half to less than 0.04, so its plate is mostly absent rows, and an absent row is a hole at ANY camera, the key's own
included.  The statement under test -- at a key's own camera the warp is the identity and has no holes -- is about a plate that is
whole, so these tests render a model of their own (the same builder, sizes and seed) whose two background density heads have
their bias raised by ``DENSE``: a background that is there on every ray, as a room's is.  Nothing else differs, and the shared
fixture model is not touched.

The drivers' guard.  A dense fog's expected depth is that of its first sample behind the background box's near face, jittered
inside the first of the 12 coarse strata: from this camera (distance 4, a box of half side 3) t_near >= 0.87 and the stratum is
(t_far - t_near) / 12 <= 0.6 long, so neighbouring pixels' depths differ by a factor below 2 out of jitter alone.  ``REL = 1``
(a factor of 2) is therefore the smallest round guard that a whole plate of THIS scene passes at its own camera; a tighter one
re-renders jitter, which is correct and costs rays (0.25: 180 of 391 pixels at the key's own pose, measured)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import reproject_common as R
import scene_edits_common as S
from instances_common import base_model
from pipeline_chain import same_bits
from stnerf_amd import hip, ops, parallel, synthetic as syn
from stnerf_amd import reproject as rp

pytestmark = pytest.mark.gpu

F = np.float32
H, W = S.H, S.W                 # 17 x 23
N = H * W
POISON = R.POISON               # a NaN pattern no kernel writes
IDS = [1.0, 2.5, 3.0]
DENSE = 4.0                     # added to the background's density biases (above)
REL, A_MIN = 1.0, 0.5           # the drivers' guard (above) and alpha floor, passed explicitly everywhere
ORBIT = 15.0


def poisoned(*shape, dtype=torch.float32):
    if dtype == torch.int64:
        return torch.full(shape, (POISON << 32) | POISON, dtype=torch.int64, device="cuda")
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(dtype)


def is_poison(x):
    return bool((x.contiguous().view(torch.int32) == POISON).all())


# ---------------------------------------------------------------------------------------- kernels against the restatement
def device_sources(srcs):
    return [(torch.from_numpy(s[0]), torch.from_numpy(s[2]), s[3], s[4], torch.from_numpy(s[5]).cuda(), torch.from_numpy(s[6]).cuda())
            for s in srcs]


def run_case(name):
    srcs, (K_d, T_d, h_d, w_d), rel = R.build_case(name)
    got = ops.reproject(device_sources(srcs), torch.from_numpy(K_d), torch.from_numpy(T_d), h_d, w_d, rel, R.Z_MIN)
    torch.cuda.synchronize()
    return got, R.oracle_case(name)


def assert_equals_oracle(got, ref, what):
    values, t, src, holes, n = got
    assert n == ref["n_holes"] and holes.dtype == torch.int32 and src.dtype == torch.int32, (what, n, ref["n_holes"])
    assert np.array_equal(src.cpu().numpy(), ref["src"]), what
    assert np.array_equal(holes.cpu().numpy(), ref["holes"]), what
    assert R.same_bits(t.cpu().numpy(), ref["t"]), what
    assert R.same_bits(values.cpu().numpy(), ref["values"]), what


def test_the_same_camera_copies_every_row():
    (values, t, src, holes, n), ref = run_case("same_camera")
    srcs = R.build_case("same_camera")[0]
    assert n == 0 and holes.shape == (0,) and torch.equal(src.cpu(), torch.arange(N, dtype=torch.int32))
    assert R.same_bits(values.cpu().numpy(), srcs[0][5])                    # bit-equal to the source
    assert_equals_oracle((values, t, src, holes, n), ref, "same_camera")


@pytest.mark.parametrize("name", ["orbit_3", "orbit_15", "dist_4_to_3", "other_K_19x29", "two_sources"] + [f"truncated_{n}" for n in (1, 63, 64, 65, 391)])
def test_bit_for_bit_against_the_restatement(name):
    got, ref = run_case(name)
    print(name, R.census(ref))
    assert_equals_oracle(got, ref, name)


def test_an_exact_tie_goes_to_the_lower_id_whatever_the_launch_order():
    got, ref = run_case("tie_twice")
    assert_equals_oracle(got, ref, "tie_twice")
    assert R.census(ref)["tie"] > 0 and int(got[2].max()) < N               # the lower id is in every src
    # the second source splatted FIRST: the same keys
    srcs, (K_d, T_d, h_d, w_d), rel = R.build_case("tie_twice")
    dev = device_sources(srcs)
    K_d, T_d = torch.from_numpy(K_d), torch.from_numpy(T_d)
    keys = ops.reproject_keys(h_d, w_d)
    for base, s in ((N, dev[1]), (0, dev[0])):
        ops.reproject_splat(keys, s[0], s[1], s[2], s[3], s[5], base, K_d, T_d, h_d, w_d, R.Z_MIN)
    torch.cuda.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), ref["keys"])
    values, t, src = ops.reproject_resolve(keys, h_d, w_d, rel, [dev[0][4], dev[1][4]])
    assert np.array_equal(src.cpu().numpy(), ref["src"]) and R.same_bits(values.cpu().numpy(), ref["values"])


def test_what_reaches_nothing_leaves_the_keys_untouched():
    """Absent rows (NaN, t <= 0, infinite), points behind the destination camera and points outside its image leave their
    targets as they were; nothing is written beyond h_d w_d."""
    K, T = R.camera(H, W)
    t, values = R.analytic_frame(K, T, H, W)
    Kt, Tt = torch.from_numpy(K), torch.from_numpy(T)

    def splat(t_src, K_d, T_d, pad=64):
        keys = poisoned(N + pad, dtype=torch.int64)
        keys[:N] = -1
        ops.reproject_splat(keys[:N], Kt, Tt, H, W, torch.from_numpy(t_src).cuda(), 0, torch.from_numpy(K_d), torch.from_numpy(T_d), H, W, R.Z_MIN)
        torch.cuda.synchronize()
        assert is_poison(keys[N:])
        return keys[:N].cpu().numpy().view(np.uint64)
    bad = t.copy()
    bad[::4], bad[1::4], bad[2::4], bad[3::4] = np.nan, 0.0, -1.0, np.inf
    K_d, T_d = R.camera(H, W, 3.0)
    assert (splat(bad, K_d, T_d) == R.EMPTY).all()
    K_b, T_b = R.camera(H, W, 0.0, -8.0)                                    # beyond the far plane, looking away: all behind
    assert (splat(t, K_b, T_b) == R.EMPTY).all()
    K_o, T_o = R.camera(H, W, 80.0)                                         # from the side: part of the points leave the image
    ref, _ = R.splat([(R.kinv_of(K), T, H, W, values, t)], K_o, T_o, H, W)
    got = splat(t, K_o, T_o)
    assert np.array_equal(got, ref) and 0 < int((ref != R.EMPTY).sum()) < N
    some = t.copy()
    some[::2] = np.nan                                                      # half the rows absent: the other half's keys only
    ref, _ = R.splat([(R.kinv_of(K), T, H, W, values, some)], K_d, T_d, H, W)
    assert np.array_equal(splat(some, K_d, T_d), ref)


def test_resolve_and_the_hole_list_write_nothing_beyond_the_view():
    srcs, (K_d, T_d, h_d, w_d), rel = R.build_case("other_K_19x29")
    ref = R.oracle_case("other_K_19x29")
    P, pad = h_d * w_d, 37
    keys = torch.from_numpy(ref["keys"].view(np.int64)).cuda()
    out = (poisoned(P + pad, R.C), poisoned(P + pad), poisoned(P + pad, dtype=torch.int32))
    ops.reproject_resolve(keys, h_d, w_d, rel, [torch.from_numpy(srcs[0][5]).cuda()], out=out)
    torch.cuda.synchronize()
    assert all(is_poison(x[P:]) for x in out)
    assert R.same_bits(out[0][:P].cpu().numpy(), ref["values"]) and np.array_equal(out[2][:P].cpu().numpy(), ref["src"])
    # a source whose rows are strided views
    wide = poisoned(N, 9)
    wide[:, 2:7] = torch.from_numpy(srcs[0][5]).cuda()
    values, _, src = ops.reproject_resolve(keys, h_d, w_d, rel, [wide[:, 2:7]])
    assert R.same_bits(values.cpu().numpy(), ref["values"])
    # the hole list: room for P entries, count in one int32; the tail of the list stays as it was
    lib = hip.lib()
    holes, n_out = poisoned(P + pad, dtype=torch.int32), poisoned(2, dtype=torch.int32)
    work = torch.empty(lib.stnerf_reproject_holes_workspace_bytes(P), dtype=torch.uint8, device="cuda")
    rc = lib.stnerf_reproject_holes(hip.dptr(src, torch.int32), P, hip.dptr(holes, torch.int32), hip.dptr(n_out, torch.int32),
                                    hip.dptr(work, torch.uint8), work.numel(), hip.stream_ptr())
    torch.cuda.synchronize()
    n = int(n_out[0])
    assert rc == hip.OK and n == ref["n_holes"] and is_poison(n_out[1:]) and is_poison(holes[n:])
    assert np.array_equal(holes[:n].cpu().numpy(), ref["holes"])


def test_every_refused_call_leaves_the_buffers_poisoned():
    """Every STNERF_EINVAL of include/stnerf.h, here with real device buffers: refused before any launch."""
    lib = hip.lib()
    K, T = R.camera(H, W)
    t, values = R.analytic_frame(K, T, H, W)
    K_d, T_d = R.camera(H, W, 3.0)
    f = lambda a: (C.c_float * a.size)(*np.asarray(a, F).reshape(-1).tolist())
    kinv, Tm, Kd, Wd, od = f(R.kinv_of(K)), f(T), f(K_d), f(R.world_to_camera(T_d)), f(T_d[:3, 3])
    t_dev, v_dev = torch.from_numpy(t).cuda(), torch.from_numpy(values).cuda()
    keys = poisoned(N, dtype=torch.int64)
    out = (poisoned(N, R.C), poisoned(N), poisoned(N, dtype=torch.int32))
    holes, n_out = poisoned(N, dtype=torch.int32), poisoned(1, dtype=torch.int32)
    work = poisoned(64)
    null = C.c_void_p(0)
    p = lambda x: C.c_void_p(x.data_ptr())

    def splat(kinv=kinv, T=Tm, h_s=H, w_s=W, t=p(t_dev), n=N, base=0, K=Kd, Wm=Wd, o=od, h_d=H, w_d=W, z=1e-6, k=p(keys)):
        return lib.stnerf_reproject_splat(kinv, T, h_s, w_s, t, n, base, K, Wm, o, h_d, w_d, z, k, hip.stream_ptr())
    for kw in (dict(kinv=None), dict(T=None), dict(t=null), dict(K=None), dict(Wm=None), dict(o=None), dict(k=null), dict(h_s=0),
               dict(h_s=1 << 16, w_s=1 << 16), dict(h_d=0), dict(h_d=1 << 16, w_d=1 << 15), dict(n=-1), dict(n=N + 1), dict(base=-1),
               dict(base=(1 << 31) - N + 1), dict(z=-1.0), dict(z=float("nan")), dict(z=float("inf"))):
        assert splat(**kw) == hip.EINVAL, kw

    def table(*recs):
        arr = (hip.ReprojectSource * max(len(recs), 1))()
        for i, (v, stride, n) in enumerate(recs):
            arr[i].values, arr[i].row_stride, arr[i].n = v, stride, n
        return arr
    vp = v_dev.data_ptr()

    def resolve(k=p(keys), h=H, w=W, rel=0.05, tab=table((vp, R.C, N)), ns=1, Cn=R.C, v=p(out[0]), tt=p(out[1]), s=p(out[2])):
        return lib.stnerf_reproject_resolve(k, h, w, rel, tab, ns, Cn, v, tt, s, hip.stream_ptr())
    for kw in (dict(k=null), dict(tab=None), dict(v=null), dict(tt=null), dict(s=null), dict(h=0), dict(h=1 << 16, w=1 << 15), dict(Cn=0),
               dict(Cn=65), dict(rel=-0.01), dict(rel=float("nan")), dict(ns=0), dict(ns=5, tab=table(*[(vp, R.C, 10)] * 5)),
               dict(tab=table((vp, R.C - 1, N))), dict(tab=table((vp, R.C, -1))), dict(tab=table((0, R.C, N))),
               dict(ns=2, tab=table((vp, R.C, (1 << 31) - 1), (vp, R.C, 1)))):
        assert resolve(**kw) == hip.EINVAL, kw
    for args in ((null, N, p(holes), p(n_out), p(work), 256), (p(out[2]), N, null, p(n_out), p(work), 256),
                 (p(out[2]), N, p(holes), null, p(work), 256), (p(out[2]), N, p(holes), p(n_out), null, 256),
                 (p(out[2]), 0, p(holes), p(n_out), p(work), 256), (p(out[2]), 1 << 31, p(holes), p(n_out), p(work), 256),
                 (p(out[2]), N, p(holes), p(n_out), p(work), 255)):
        assert lib.stnerf_reproject_holes(*args, hip.stream_ptr()) == hip.EINVAL, args
    torch.cuda.synchronize()
    assert all(is_poison(x) for x in (keys,) + out + (holes, n_out, work))
    # and the Python front refuses more than four sources, and rows that are not (n, C)
    src = (torch.from_numpy(K), torch.from_numpy(T), H, W, v_dev, t_dev)
    with pytest.raises(ValueError, match="sources"):
        ops.reproject([src] * 5, torch.from_numpy(K_d), torch.from_numpy(T_d), H, W, 0.05)
    with pytest.raises(ValueError, match="sources"):
        ops.reproject([], torch.from_numpy(K_d), torch.from_numpy(T_d), H, W, 0.05)
    with pytest.raises(ValueError):
        ops.reproject([src[:5] + (t_dev[:-1],)], torch.from_numpy(K_d), torch.from_numpy(T_d), H, W, 0.05)


# ---------------------------------------------------------------------------------------- the drivers
@pytest.fixture(scope="module")
def dense_model():
    """The L = 2 model of tests/test_gpu_scene_edits_oracle.py (``instances_common.base_model``, its sizes, seed and launch cap),
    built for this module alone, its background made dense (the module docstring says why).  The device's draws, no replay."""
    model = base_model(2)
    with torch.no_grad():
        model.bkgd_spacenet.density_net[0].bias.add_(DENSE)
        model.bkgd_spacenet_fine.density_net[0].bias.add_(DENSE)
    model = model.cuda()
    bk, per = syn.scene_boxes(2)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.train(False)
    model.coarse_ray_sample, model.fine_ray_sample = 12, 6
    model.set_precision("bf16x3")
    model.max_rays_per_launch = S.CAP
    model.seed, model.fresh_draws_per_call, model.replay = 11, False, None
    return model


@pytest.fixture
def model(dense_model):
    m = dense_model
    yield m
    m.train(False)
    m.set_background_cache(None)
    for i in range(m.total_layers):
        m.show_layer(i)
    m.shift = None
    m.view_key, m.view_frame_ids = None, None
    m.seed, m.fresh_draws_per_call = 11, False


SPEC = rp.ReprojectSpec(3, REL, A_MIN)


def background_only(model, rays):
    """Layer 0 alone, by hand: the performers hidden, ``render_rays_raw``, the performers shown again."""
    for i in range(1, model.total_layers):
        model.hide_layer(i)
    with torch.no_grad():
        mixed = model.render_rays_raw(rays)[2][:, 0]                       # (layer 0's own output: the layer composited alone)
    for i in range(1, model.total_layers):
        model.show_layer(i)
    return mixed


def rows_by_hand(mixed, a_min=A_MIN):
    """The plate rows in torch, restated: straight colour, alpha, depth over alpha; absent below a_min."""
    a = mixed[:, 4:5]
    rows = torch.cat([mixed[:, 0:1] / a, mixed[:, 1:2] / a, mixed[:, 2:3] / a, a, mixed[:, 3:4] / a], 1)
    gone = torch.tensor([0.0, 0.0, 0.0, 0.0, float("nan")], device=mixed.device)
    return torch.where(a >= a_min, rows, gone.expand_as(rows))


def occluded_by_hand(model, rays, rows):
    model.hide_layer(0)
    with torch.no_grad():
        out = model.render_rays_occluded(rays, rows)
    model.show_layer(0)
    return out


def flat(out):
    """(5-tuple, scene, occluded) -> a list of every tensor in it, in a fixed order."""
    five, scene, occ = out
    xs = list(five[0]) + list(five[1]) + [x for t in five[2] for x in t] + [x for t in five[3] for x in t] + list(five[4])
    xs += [x for t in scene for x in t] + list(occ["mixed"]) + [x for t in occ["scene"] for x in t] + list(occ["share"])
    return xs


def assert_same_outputs(a, b):
    xa, xb = flat(a), flat(b)
    assert len(xa) == len(xb)
    for i, (x, y) in enumerate(zip(xa, xb)):
        assert x.dtype == y.dtype and (torch.equal(x, y) if x.dtype == torch.bool else same_bits(x, y)), i


def test_a_keys_own_pose_is_the_plate_composited_by_hand(model):
    K, T = syn.camera(H, W, ORBIT)
    plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC, index=0)
    rays = ops.generate_rays(K, T, H, W, frame_ids=IDS)
    rows = rows_by_hand(background_only(model, rays))
    assert same_bits(plate.rows, rows) and int(torch.isnan(plate.t).sum()) == 0        # a whole plate
    five, scene, occluded, stats = parallel.render_view_reprojected(model, K, T, H, W, IDS, [plate], SPEC)
    print("own pose:", stats)
    assert stats == dict(holes=0, reused=N, rays_background=0, keys=(0,))
    # (the kernels at the key's own camera: every pixel from itself, no hole, the depth back within a rounding or two)
    values, t, src, holes, n = ops.reproject([plate.source()], K, T, H, W, REL)
    assert n == 0 and torch.equal(src.cpu(), torch.arange(N, dtype=torch.int32)) and same_bits(values, plate.rows)
    # (p = t d + o is rounded at |o| = 4: half an ulp of 4, 2.4e-7, per component; e = p - o is exact; the norm adds a few ulps of t)
    assert float((t - plate.t).abs().max()) <= 1e-6
    assert_same_outputs((five, scene, occluded), occluded_by_hand(model, rays, rows))
    assert float(occluded["mixed"][2].min()) > 0.0 and model.display_layers == {0: 1, 1: 1, 2: 1} and model.seed == 11
    torch.cuda.synchronize()


def test_an_in_between_pose_renders_its_holes_and_reuses_the_rest(model):
    K, T = syn.camera(H, W, ORBIT)
    K2, T2 = syn.camera(H, W, ORBIT + 3.0)
    plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC, index=0)
    five, scene, occluded, stats = parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate], SPEC)
    print("3 degrees on:", stats)
    assert stats["holes"] + stats["reused"] == N and 0 < stats["holes"] < N and stats["rays_background"] == stats["holes"]
    # the same by hand: the warp, the holes' pixel list rendered with layer 0 alone, the finished plate as the occluder
    values, t, src, holes, n = ops.reproject([plate.source()], K2, T2, H, W, REL)
    assert n == stats["holes"] and torch.equal(holes.long(), torch.nonzero(src < 0).flatten())
    rows, got_holes, got_n, warped = rp.warp_plates(model, K2, T2, H, W, IDS, [plate], SPEC)
    assert got_n == n and torch.equal(got_holes, holes) and all(same_bits(a.float(), b.float()) for a, b in zip(warped, (values, t, src)))
    hole_rows = rows_by_hand(background_only(model, ops.generate_rays(K2, T2, H, W, frame_ids=IDS, pixels=holes)))
    assert same_bits(rows[holes.long()], hole_rows)
    kept = src >= 0
    assert same_bits(rows[kept][:, :4], values[kept][:, :4]) and same_bits(rows[kept][:, 4], t[kept])
    assert_same_outputs((five, scene, occluded), occluded_by_hand(model, ops.generate_rays(K2, T2, H, W, frame_ids=IDS), rows))
    # two keys, one on either side, leave fewer holes than one
    K3, T3 = syn.camera(H, W, ORBIT + 6.0)
    plate3 = rp.BackgroundPlate.render(model, K3, T3, H, W, IDS, SPEC, index=2)
    _, _, _, both = parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate, plate3], SPEC)
    print("between two keys:", both)
    assert both["keys"] == (0, 2) and both["holes"] <= stats["holes"]
    torch.cuda.synchronize()


def renderer(model, angles, **kw):
    from stnerf_amd.render import LayeredNeuralRenderer
    cams = [syn.camera(H, W, a) for a in angles]
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.stack([torch.as_tensor(T) for _, T in cams]), gt_Ks=[K for K, _ in cams], **kw)
    r.set_path_gt_poses()
    assert len(r.poses) == len(angles)
    return r


def test_key_every_one_is_the_per_pose_call_with_a_fresh_plate(model):
    from stnerf_amd.render.render_pose import render_pose
    r = renderer(model, [ORBIT + 2.0 * i for i in range(4)], reproject=dict(key_every=1, rel=REL, a_min=A_MIN))
    seen = []
    r.render_path(on_frame=lambda idx, c, d, cl, dl, reprojected=None: seen.append((idx, c.clone(), d.clone(), reprojected)))
    assert len(seen) == 4 and len(r.reproject_stats) == 4 and len(r.images) == 4
    for k in range(4):
        ids = [0.0] * 3
        for layer, frame in r.layer_frame_pairs[k]:
            ids[layer] = float(frame)
        plates = [rp.BackgroundPlate.render(model, r.Ks[j], r.poses[j], H, W, ids, r.reproject, index=j) for j in (k, k + 1) if j < 4]
        c, d, cl, dl, st = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0, reproject=(r.reproject, plates))
        idx, sc, sd, got = seen[k]
        assert idx == k and same_bits(sc, c) and same_bits(sd, d) and same_bits(sc, st["passes"]["color_occluded"])
        assert got["keys"] == st["keys"] == tuple(j for j in (k, k + 1) if j < 4)
        assert all(got[x] == st[x] == r.reproject_stats[k][x] for x in ("holes", "reused", "rays_background"))
        assert r.reproject_stats[k]["keys_rendered"] == (2 if k == 0 else 1 if k < 3 else 0)
    assert r.reproject_stats[3]["holes"] == 0                               # the last key alone, at its own pose
    torch.cuda.synchronize()


def test_key_every_three_over_five_poses_uses_two_keys(model):
    r = renderer(model, [ORBIT + 3.0 * i for i in range(5)], reproject=SPEC)
    seen = []
    r.render_path(on_frame=lambda idx, c, d, cl, dl, reprojected=None: seen.append((idx, reprojected)))
    stats = r.reproject_stats
    print([{k: v for k, v in s.items()} for s in stats])
    assert [s["keys"] for s in stats] == [(0, 3), (0, 3), (0, 3), (3,), (3,)]
    assert [s["keys_rendered"] for s in stats] == [2, 0, 0, 0, 0] and sorted(r._plates) == [3]
    assert all(s["holes"] + s["reused"] == N and s["rays_background"] == s["holes"] for s in stats)
    assert stats[3]["holes"] == 0 and stats[4]["holes"] > 0                 # key 3 alone: at its own pose, and 3 degrees on
    assert [i for i, _ in seen] == list(range(5)) and all(st is not None and st["keys"] == stats[i]["keys"] and "passes" in st for i, st in seen)
    # a frame under another background re-keys instead of failing: layer 0 shifted between two paths
    model.shift = [[0.05, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    try:
        stale = dict(r._plates)
        with pytest.raises(ValueError, match="another background"):
            parallel.render_view_reprojected(model, r.Ks[4], r.poses[4], H, W, IDS, [stale[3]], SPEC)
        plates, rendered = r._key_plates(4, 0, 0)
        assert rendered == 1 and plates[0] is not stale[3] and plates[0].index == 3
    finally:
        model.shift = None
    torch.cuda.synchronize()


def test_the_model_is_as_before_after_success_and_after_an_exception(model):
    K, T = syn.camera(H, W, ORBIT)
    K2, T2 = syn.camera(H, W, ORBIT + 3.0)
    model.hide_layer(2)
    model.view_key, model.view_frame_ids = ("mine",), (1.0,)
    model.fresh_draws_per_call = True
    try:
        want = ({0: 1, 1: 1, 2: 0}, ("mine",), (1.0,), 11)
        state = lambda: (dict(model.display_layers), model.view_key, model.view_frame_ids, model.seed)
        plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC)
        assert state() == want
        parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate], SPEC)
        assert state() == want
        # an exception raised inside each of the two renders
        boom = RuntimeError("boom")
        real = model.render_rays_raw
        model.render_rays_raw = lambda *a, **k: (_ for _ in ()).throw(boom)
        try:
            with pytest.raises(RuntimeError, match="boom"):
                parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate], SPEC)
            with pytest.raises(RuntimeError, match="boom"):
                rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC)
        finally:
            del model.render_rays_raw
        assert model.render_rays_raw.__func__ is real.__func__ and state() == want
        real_occ = model.render_rays_occluded
        model.render_rays_occluded = lambda *a, **k: (_ for _ in ()).throw(boom)
        try:
            with pytest.raises(RuntimeError, match="boom"):
                parallel.render_view_reprojected(model, K2, T2, H, W, IDS, [plate], SPEC)
        finally:
            del model.render_rays_occluded
        assert model.render_rays_occluded.__func__ is real_occ.__func__ and state() == want
    finally:
        model.view_key, model.view_frame_ids = None, None
    torch.cuda.synchronize()


def test_every_refusal(model):
    from stnerf_amd.lens import Lens
    from stnerf_amd.render.render_pose import render_pose
    K, T = syn.camera(H, W, ORBIT)
    plate = rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC)
    call = lambda **kw: parallel.render_view_reprojected(model, K, T, H, W, IDS, [plate], SPEC, **kw)
    pairs = list(enumerate(IDS))
    # more than one rank (as ``scene``)
    real = parallel.active_group
    parallel.active_group = lambda m=None: (0, 2, None)
    try:
        with pytest.raises(RuntimeError, match="more than one rank"):
            call()
        with pytest.raises(RuntimeError, match="more than one rank"):
            rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC)
    finally:
        parallel.active_group = real
    # training mode, which is the op-by-op path
    model.train(True)
    try:
        with torch.enable_grad():
            with pytest.raises(RuntimeError, match="training mode.*op-by-op"):
                call()
            with pytest.raises(RuntimeError, match="training mode"):
                rp.BackgroundPlate.render(model, K, T, H, W, IDS, SPEC)
    finally:
        model.train(False)
    # accumulate=, a lens, an occluder of the caller's, only_coarse
    with pytest.raises(ValueError, match="accumulate"):
        render_pose(model, T, K, H, W, pairs, 20.0, reproject=(SPEC, [plate]), accumulate=dict(max_spp=2))
    lens = Lens(k1=0.1)
    with pytest.raises(ValueError, match="lens"):
        call(lens=lens)
    with pytest.raises(ValueError, match="lens"):
        render_pose(model, T, K, H, W, pairs, 20.0, reproject=(SPEC, [plate]), lens=lens)
    with pytest.raises(ValueError, match="occluder"):
        call(occluder=torch.zeros(N, 5, device="cuda"))
    with pytest.raises(ValueError, match="occluder"):
        render_pose(model, T, K, H, W, pairs, 20.0, reproject=(SPEC, [plate]), occluder=(torch.zeros(H, W, 4), torch.ones(H, W)))
    with pytest.raises(ValueError, match="only_coarse"):
        call(only_coarse=True)
    with pytest.raises(ValueError, match="scene_passes"):
        render_pose(model, T, K, H, W, pairs, 20.0, reproject=(SPEC, [plate]), scene_passes=True)
    # a hidden background, no plate, a plate of another background
    model.hide_layer(0)
    with pytest.raises(ValueError, match="layer 0 hidden"):
        call()
    model.show_layer(0)
    with pytest.raises(ValueError, match="no plate"):
        parallel.render_view_reprojected(model, K, T, H, W, IDS, [], SPEC)
    model.seed = 12
    with pytest.raises(ValueError, match="another background"):
        call()
    model.seed = 11
    # the renderer refuses the same combinations when it is built
    for kw, word in ((dict(accumulate=dict(max_spp=2)), "accumulate"), (dict(occluder=lambda i, p, k: None), "occluder"),
                     (dict(lens=lens), "lens"), (dict(scene_passes=True), "scene_passes")):
        with pytest.raises(ValueError, match=word):
            renderer(model, [ORBIT], reproject=SPEC, **kw)
    assert model.display_layers == {0: 1, 1: 1, 2: 1} and model.seed == 11
    torch.cuda.synchronize()


def test_without_reproject_the_renderer_renders_what_it_did(model):
    from stnerf_amd.render.render_pose import render_pose
    r = renderer(model, [ORBIT])
    assert r.reproject is None
    seen = []
    r.render_path(on_frame=lambda idx, c, d, cl, dl: seen.append((c.clone(), d.clone(), [x.clone() for x in cl])))
    c, d, cl, dl = render_pose(model, r.poses[0], r.Ks[0], H, W, r.layer_frame_pairs[0], r.far, 0, 0)
    assert same_bits(seen[0][0], c) and same_bits(seen[0][1], d) and all(same_bits(a, b) for a, b in zip(seen[0][2], cl))
    assert r.reproject_stats == [] and r._plates == {}
    torch.cuda.synchronize()
