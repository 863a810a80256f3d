"""The lens model in ray generation on the MI355X (csrc/lens.hip): ``stnerf_generate_rays_lens`` against the
numpy oracle of tests/lens_common.py, bit for bit; then the drivers (``parallel.render_view(lens=)``,
``parallel.render_view_accumulated(lens=)``), ``render_pose(lens=)`` and the renderer's ``lens=`` on the small model and camera of
tests/test_gpu_accumulate.py (17 x 23 = 391 rays), in both arithmetics, the seed set equal before each side."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import accumulate_common as A
import lens_common as LC
import occluder_common as OCL
import occupancy_common as OCC
import scene_edits_common as S
import test_gpu_scene_edits_oracle as SE
from pipeline_chain import bits, detach_models, same_bits
from stnerf_amd import hip, ops, parallel, synthetic as syn
from stnerf_amd.accumulate import AccumulateSpec
from stnerf_amd.lens import Lens

pytestmark = pytest.mark.gpu

F = np.float32
H, W = S.H, S.W                 # 17 x 23
N = H * W
POISON = 0x7FC0BEEF             # a NaN pattern no kernel writes
IDS3 = [1.0, 2.5, 3.0]
KEYS = (0, 0x9E3779B9)


@pytest.fixture(autouse=True)
def detach():
    yield
    detach_models()


def eq(a, b):
    """The same dtype, shape and bytes."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def camera(h=H, w=W, f=None, orbit=15.0):
    K, T = syn.camera(h, w, orbit)
    if f is not None:
        K[0, 0] = K[1, 1] = f
    return K, T, torch.inverse(K.to(torch.float32)).numpy(), torch.as_tensor(T, dtype=torch.float32).numpy()


# ---------------------------------------------------------------------------------------- the entry
def raw_lens(cam, h, w, pixels, n, du=0.0, dv=0.0, rec=None, pad=0, fids=IDS3, rows=None):
    """stnerf_generate_rays_lens itself, on a poisoned buffer of ``rows`` >= n rows of 6 + cols + pad floats."""
    _, _, kinv, Tm = cam
    rows = n if rows is None else rows
    out = torch.full((rows, 6 + len(fids) + pad), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
    kin, tin, fin = (C.c_float * 9)(*kinv.reshape(-1).tolist()), (C.c_float * 16)(*Tm.reshape(-1).tolist()), (C.c_float * len(fids))(*fids)
    rc = hip.lib().stnerf_generate_rays_lens(kin, tin, h, w, hip.dptr(pixels, torch.int32), n, du, dv, None if rec is None else C.byref(rec),
                                             fin, len(fids), hip.dptr(out), out.shape[1], hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def lens_cases(focus):
    """(name, record fields, table | None, oracle keywords): distortion only (the four sets), lens only (n_points 1, 3, 8; every
    phase; with and without decorrelate; two keys), and both together."""
    out = []
    for c in LC.SETS:
        out.append((f"distort {c}", dict(distort=1, k1=c[0], k2=c[1], k3=c[2], p1=c[3], p2=c[4]), None, dict(coeffs=c)))
    for m in (1, 3, 8):
        tab = LC.table(m, 0.07) + (F(0.01) if m == 1 else F(0))          # (one point: off the centre, so that the lens branch runs)
        for phase in range(m):
            for dec in (0, 1):
                for key in KEYS if dec else KEYS[:1]:
                    out.append((f"lens {m} points, phase {phase}, decorrelate {dec}, key {key:#x}",
                                dict(n_points=m, phase=phase, decorrelate=dec, key=key, focus=focus), tab,
                                dict(points=tab, phase=phase, decorrelate=bool(dec), key=key, focus=focus)))
    tab = LC.table(8, 0.07)
    for c, phase, dec in ((LC.SETS[0], 3, 1), (LC.SETS[1], 5, 0), (LC.SETS[3], 7, 1)):
        out.append((f"both {c}, phase {phase}, decorrelate {dec}",
                    dict(distort=1, k1=c[0], k2=c[1], k3=c[2], p1=c[3], p2=c[4], n_points=8, phase=phase, decorrelate=dec, key=KEYS[1], focus=focus),
                    tab, dict(coeffs=c, points=tab, phase=phase, decorrelate=bool(dec), key=KEYS[1], focus=focus)))
    return out


def check_entry(cam, h, w, pix, n, du, dv, pads=(0, 1)):
    """Every case of ``lens_cases`` through the entry on the list ``pix`` (None: the contiguous pixels 0..n-1), against the oracle."""
    _, _, kinv, Tm = cam
    listed = np.arange(n) if pix is None else pix
    plist = None if pix is None else dev_i32(pix)
    worst = 0.0
    for name, fields, tab, kw in lens_cases(4.0):
        dtab = None if tab is None else torch.from_numpy(tab).cuda()
        rec = hip.LensRecord(**fields)
        if dtab is not None:
            rec.points = dtab.data_ptr()
        want = LC.rays_of_lens(kinv, Tm, w, listed, du, dv, IDS3, **kw)
        for pad in pads:
            rc, out = raw_lens(cam, h, w, plist, n, du, dv, rec, pad, rows=n + 2)
            assert rc == hip.OK, (name, hip.last_error())
            got = out.cpu().numpy()
            assert LC.same_bits(got[:n, :9], want), (name, pad, float(np.nanmax(np.abs(got[:n, :9] - want))))
            assert (got[:n, 9:].view(np.int32) == POISON).all() and (got[n:].view(np.int32) == POISON).all(), (name, pad)
        pin = LC.rays_of_lens(kinv, Tm, w, listed, du, dv, IDS3)
        worst = max(worst, float(np.nanmax(np.abs(want[:, :6] - pin[:, :6]))))
    assert worst > 1e-3                                                       # the lens moves the rays: not the plain rows
    return worst


def pixel_list(n, order):
    if order == "null":
        return None
    pix = np.random.RandomState(100 + n).choice(N, n, replace=False)
    return np.sort(pix) if order == "ascending" else pix


@pytest.mark.parametrize("order", ["ascending", "shuffled", "null"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 391])
def test_the_entry_equals_the_numpy_restatement(n, order):
    """Zero offset and a non-zero one, row strides 6 + cols and 7 + cols, every lens case."""
    cam = camera()
    check_entry(cam, H, W, pixel_list(n, order), n, 0.0, 0.0)
    worst = check_entry(cam, H, W, pixel_list(n, order), n, 0.25, -0.375, pads=(1,))
    print(f"n = {n}, {order}: the lens moves a ray component by up to {worst:.3f}")


def test_the_entry_at_1080p():
    """f = 1500 over 1080 x 1920 through a 64-entry list of corner, edge and centre pixels (pixel indices up to 2,073,599)."""
    h, w = 1080, 1920
    cam = camera(h, w, f=1500.0, orbit=40.0)
    cols = [0, 1, 2, w // 2 - 1, w // 2, w - 3, w - 2, w - 1]
    rows = [0, 1, h // 3, h // 2 - 1, h // 2, h - 3, h - 2, h - 1]
    pix = np.array([r * w + c for r in rows for c in cols], np.int64)
    assert len(pix) == 64 and pix.max() == h * w - 1
    check_entry(cam, h, w, np.random.RandomState(5).permutation(pix), 64, 0.0, 0.0)
    check_entry(cam, h, w, pix, 64, -0.5, 0.3125, pads=(0,))


def test_a_table_row_at_the_lens_centre_is_the_pinhole_ray_and_an_entry_outside_the_view_is_skipped():
    cam = camera()
    _, _, kinv, Tm = cam
    tab = np.array([[0.05, -0.02], [0.0, 0.0], [-0.03, 0.06]], F)            # the centre at a NON-zero phase
    dtab = torch.from_numpy(tab).cuda()
    pix = np.arange(N)
    plain = raw_lens(cam, H, W, None, N)[1]
    for phase, dec in ((1, 0), (0, 1), (1, 1), (2, 1)):
        rec = hip.LensRecord(points=dtab.data_ptr(), n_points=3, phase=phase, decorrelate=dec, key=7, focus=4.0)
        rc, out = raw_lens(cam, H, W, None, N, rec=rec)
        j = LC.table_rows(pix, 3, phase, bool(dec), 7)
        centre = torch.from_numpy(j == 1).cuda()
        assert rc == hip.OK and bool(centre.any()) and (dec == 0 or not bool(centre.all()))
        assert same_bits(out[centre], plain[centre])                         # per row: the pinhole operations and nothing else
        assert not bool((bits(out[~centre][:, :6]) == bits(plain[~centre][:, :6])).all(1).any())
        assert LC.same_bits(out.cpu().numpy(), LC.rays_of_lens(kinv, Tm, W, pix, 0.0, 0.0, IDS3, points=tab, phase=phase, decorrelate=bool(dec),
                                                              key=7, focus=4.0))
    # a list entry outside [0, h w) leaves its row unwritten
    lst = np.array([5, -1, 390, 391, 7, 1 << 30], np.int32)
    rec = hip.LensRecord(distort=1, k1=-0.1, p1=0.001, points=dtab.data_ptr(), n_points=3, phase=2, decorrelate=1, focus=4.0)
    rc, out = raw_lens(cam, H, W, dev_i32(lst), len(lst), 0.25, -0.25, rec)
    assert rc == hip.OK
    written = ~(bits(out) == POISON).all(1).cpu().numpy()
    assert written.tolist() == [True, False, True, False, True, False]
    want = LC.rays_of_lens(kinv, Tm, W, lst[written], 0.25, -0.25, IDS3, coeffs=(-0.1, 0.0, 0.0, 0.001, 0.0), points=tab, phase=2, decorrelate=True,
                           focus=4.0)
    assert LC.same_bits(out.cpu().numpy()[written], want)
    # what the host can prove wrong is an error code before any launch (the buffer stays poisoned)
    for bad in (hip.LensRecord(distort=1, k1=float("nan")), hip.LensRecord(points=dtab.data_ptr(), n_points=3, phase=3, focus=4.0),
                hip.LensRecord(points=dtab.data_ptr(), n_points=3, phase=0, focus=-4.0)):
        rc, out = raw_lens(cam, H, W, None, 8, rec=bad)
        assert rc == hip.EINVAL and bool((bits(out) == POISON).all())


@pytest.mark.parametrize("n", [1, 65, 391])
def test_a_disabled_record_and_a_null_record_are_the_pixel_list_entry(n):
    cam = camera()
    K, T = cam[:2]
    kin, tin, fin = (C.c_float * 9)(*cam[2].reshape(-1).tolist()), (C.c_float * 16)(*cam[3].reshape(-1).tolist()), (C.c_float * 3)(*IDS3)
    for pix, off in ((None, (0.0, 0.0)), (pixel_list(n, "shuffled"), (0.25, -0.5))):
        want = torch.full((n, 9), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        assert hip.lib().stnerf_generate_rays_list(kin, tin, H, W, hip.dptr(None if pix is None else dev_i32(pix), torch.int32), n, off[0], off[1], fin,
                                                   3, hip.dptr(want), 9, hip.stream_ptr()) == hip.OK
        for rec in (None, hip.LensRecord(), hip.LensRecord(k1=-0.3, focus=2.0, n_points=4, phase=9)):     # distort == 0, points == NULL
            rc, out = raw_lens(cam, H, W, None if pix is None else dev_i32(pix), n, off[0], off[1], rec)
            assert rc == hip.OK and torch.equal(out, want)
        for lens in (None, Lens(), Lens(focus=3.0, key=5, decorrelate=False), dict()):
            got = ops.generate_rays(K, T, H, W, frame_ids=IDS3, n=n, pixels=None if pix is None else dev_i32(pix), offset=off, lens=lens)
            assert torch.equal(got, want)
    assert torch.equal(ops.generate_rays(K, T, H, W, frame_ids=IDS3, lens=Lens()), ops.generate_rays(K, T, H, W, frame_ids=IDS3))
    # and ops.generate_rays(lens=) is the entry: the record it builds from a Lens
    lens = Lens(*LC.SETS[0], aperture=0.07, focus=4.0, key=KEYS[1])
    tab = lens.table(8)
    got = ops.generate_rays(K, T, H, W, frame_ids=IDS3, lens=lens, lens_phase=3, lens_points=torch.from_numpy(tab).cuda(), offset=(0.25, 0.0))
    want = LC.rays_of_lens(cam[2], cam[3], W, np.arange(N), 0.25, 0.0, IDS3, coeffs=LC.SETS[0], points=LC.table(8, 0.07), phase=3, decorrelate=True,
                           key=KEYS[1], focus=4.0)
    assert LC.same_bits(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="phase"):
        ops.generate_rays(K, T, H, W, lens=lens, lens_phase=8, lens_points=torch.from_numpy(tab).cuda())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- the drivers
THR, BTHR, CHUNCKS = 0.05, 0.02, 64
MILD = LC.SETS[0]
FOCUS, APERTURE = 4.0, 0.05


def scene(precision):
    """The model, camera and frame ids of tests/test_gpu_accumulate.py's driver tests, its draws the device's."""
    case = OCC.plain_case(chunk=S.N, thr=1e-4, bthr=0.0)
    ids = [float(x) for x in case["groups"][0][1]]
    K, T = syn.camera(S.H, S.W, case["orbit"])
    model = SE.make_model(case, precision)
    model.replay = None
    return model, K, T, ids


def oracle_rays(K, T, ids, p=0, lens=None, max_spp=1, pix=None, offset=(0.0, 0.0), frame_ids=None):
    """The oracle's rays of pass p through ``lens`` (the fields of a Lens, read here; the table restated by lens_common)."""
    kinv, Tm = torch.inverse(K.to(torch.float32)).numpy(), torch.as_tensor(T, dtype=torch.float32).numpy()
    kw = {}
    if lens is not None and lens.distorts:
        kw["coeffs"] = lens.coefficients
    if lens is not None and lens.aperture > 0:
        kw.update(points=LC.table(max_spp, lens.aperture), phase=p, decorrelate=lens.decorrelate, key=lens.key, focus=lens.focus)
    rays = LC.rays_of_lens(kinv, Tm, W, np.arange(N) if pix is None else pix, offset[0], offset[1], ids if frame_ids is None else frame_ids, **kw)
    return torch.from_numpy(rays).cuda()


def flat(out):
    return [t for part in (out[0], out[1], *out[2], *out[3]) for t in part if t is not None] + list(out[4])


def means_of(out):
    fine, coarse, layers, coarse_layers, masks = out
    assert coarse is None and coarse_layers is None
    return torch.cat(list(fine) + [x for t in layers for x in t], 1)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_no_lens_and_a_disabled_lens_are_todays_outputs(precision):
    model, K, T, ids = scene(precision)
    model.seed = 11
    today = flat(parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS))
    spec = AccumulateSpec(3, 2, 0.01, shutter=0.5, frame_range=(1.0, 3.0))
    model.seed = 11
    today_acc, today_stats = parallel.render_view_accumulated(model, K, T, H, W, ids, spec, THR, BTHR, chuncks=CHUNCKS)
    for lens in (None, Lens(), dict(focus=3.0)):
        model.seed = 11
        got = flat(parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, lens=lens))
        assert len(got) == len(today) and all(eq(a, b) for a, b in zip(got, today))
        model.seed = 11
        got_acc, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, spec, THR, BTHR, chuncks=CHUNCKS, lens=lens)
        assert same_bits(means_of(got_acc), means_of(today_acc)) and torch.equal(stats["spp"], today_stats["spp"])
        assert (stats["passes"], stats["rays_rendered"]) == (today_stats["passes"], today_stats["rays_rendered"])
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_a_distorting_lens_renders_the_oracles_rays(precision):
    """``render_view(lens=)`` == ``layered_batchify_ray`` on the oracle's rays; with ``scene=True`` == ``render_rays_scene`` and with an
    occluder == ``render_rays_occluded`` on those rays."""
    from stnerf_amd.utils.batchify_rays import layered_batchify_ray
    model, K, T, ids = scene(precision)
    lens = Lens(*MILD)
    rays = oracle_rays(K, T, ids, lens=lens)
    assert not torch.equal(rays, ops.generate_rays(K, T, H, W, frame_ids=ids))
    model.seed = 11
    got = flat(parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, lens=lens))
    model.seed = 11
    plain = flat(parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS))
    model.seed = 11
    with torch.no_grad():
        want = flat(layered_batchify_ray(model, rays, None, None, chuncks=CHUNCKS, density_threshold=THR, bkgd_density_threshold=BTHR))
    assert len(got) == len(want) and all(eq(a, b) for a, b in zip(got, want)) and not eq(got[0], plain[0])
    # scene passes
    model.seed = 11
    out, passes = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, scene=True, lens=dict(zip(("k1", "k2", "k3", "p1", "p2"), MILD)))
    model.seed = 11
    with torch.no_grad():
        want_out, want_passes = model.render_rays_scene(rays, False, THR, BTHR, ref_chunk=CHUNCKS)
    assert all(eq(a, b) for a, b in zip(flat(out), flat(want_out)))
    assert len(passes) == len(want_passes) and all(eq(a, b) for x, y in zip(passes, want_passes) for a, b in zip(x, y))
    # an occluder
    occ = torch.from_numpy(OCL.case_occluder()).cuda()
    model.seed = 11
    out, passes, occluded = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, occluder=occ, lens=lens)
    model.seed = 11
    with torch.no_grad():
        want_out, want_passes, want_occluded = model.render_rays_occluded(rays, occ, False, THR, BTHR, ref_chunk=CHUNCKS, stops=False)
    assert all(eq(a, b) for a, b in zip(flat(out), flat(want_out)))
    assert all(eq(a, b) for x, y in zip(passes, want_passes) for a, b in zip(x, y))
    assert all(eq(a, b) for a, b in zip(occluded["mixed"], want_occluded["mixed"])) and all(eq(a, b) for a, b in zip(occluded["share"], want_occluded["share"]))
    assert all(eq(a, b) for x, y in zip(occluded["scene"], want_occluded["scene"]) for a, b in zip(x, y))
    torch.cuda.synchronize()


def oracle_pass(model, K, T, ids, s0, p, shutters, lens, max_spp, pix=None):
    """Pass p rendered on the ORACLE's rays: the schedule's offset and frame ids, seed s0 + p, the view's thresholds."""
    model.seed = s0 + p
    rays = oracle_rays(K, T, ids, p, lens, max_spp, pix, tuple(float(x) for x in A.offset(p)), [float(x) for x in A.layer_frame_ids(p, ids, shutters)])
    with torch.no_grad():
        raw = model.render_rays_raw(rays, False, THR, BTHR, ref_chunk=CHUNCKS)
    return parallel.pack_outputs(raw, "fine")[:, :-1].cpu().numpy()


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_fixed_spp_through_an_aperture_is_the_oracles_mean_of_passes_on_oracle_rays(precision):
    model, K, T, ids = scene(precision)
    l = model.total_layers
    shutters = [0.0, 0.8] + [0.0] * (l - 2)
    for lens in (Lens(aperture=APERTURE, focus=FOCUS), Lens(*MILD, aperture=APERTURE, focus=FOCUS, decorrelate=False, key=3)):
        want = A.State(N, 5 + 5 * l, 3)
        rows = []
        for p in range(3):
            rows.append(oracle_pass(model, K, T, ids, 11, p, shutters, lens, 3))
            A.update(want, rows[-1])
        assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
        model.seed = 11
        out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(3, shutter=shutters), THR, BTHR, chuncks=CHUNCKS, lens=lens)
        torch.cuda.synchronize()
        assert model.seed == 11
        assert A.same_bits(means_of(out).cpu().numpy(), want.mean)
        assert bool((stats["spp"] == 3).all()) and stats["passes"] == 3 and stats["rays_rendered"] == 3 * N
        # the aperture shows: another frame than the pinhole's three passes
        model.seed = 11
        pin, _ = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(3, shutter=shutters), THR, BTHR, chuncks=CHUNCKS)
        assert not same_bits(means_of(pin), means_of(out))


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_adaptive_spp_through_a_lens_replays_as_the_op_level_loop(precision):
    """(min 2, max 4), tol = the median standard error after two passes: the loop replayed with ``ops.generate_rays(lens=, lens_phase=,
    lens_points=)`` and the oracle's update and select; the driver's means, spp map, pass count and ray count must be those."""
    model, K, T, ids = scene(precision)
    l = model.total_layers
    shutters = [0.0, 0.8] + [0.0] * (l - 2)
    lens = Lens(*MILD, aperture=APERTURE, focus=FOCUS, key=KEYS[1])
    table = torch.from_numpy(lens.table(4)).cuda()

    def op_pass(p, pix=None):
        model.seed = 11 + p
        rays = ops.generate_rays(K, T, H, W, frame_ids=[float(x) for x in A.layer_frame_ids(p, ids, shutters)], offset=tuple(float(x) for x in A.offset(p)),
                                 pixels=None if pix is None else dev_i32(pix), lens=lens, lens_phase=p, lens_points=table)
        want = oracle_rays(K, T, ids, p, lens, 4, pix, tuple(float(x) for x in A.offset(p)), [float(x) for x in A.layer_frame_ids(p, ids, shutters)])
        assert same_bits(rays, want)
        with torch.no_grad():
            raw = model.render_rays_raw(rays, False, THR, BTHR, ref_chunk=CHUNCKS)
        return parallel.pack_outputs(raw, "fine")[:, :-1].cpu().numpy()

    want = A.State(N, 5 + 5 * l, 3)
    for p in range(2):
        A.update(want, op_pass(p))
    tol = float(np.median(np.sqrt(A.variance_of_mean(want)).max(1)))
    assert tol > 0.0
    passes, rendered = 2, 2 * N
    while passes < 4:
        pix = A.select(want, 2, 4, tol)
        if len(pix) == 0:
            break
        A.update(want, op_pass(passes, pix), pix)
        rendered += len(pix)
        passes += 1
    print(f"{precision}: tol {tol:.3e}, spp histogram {np.bincount(want.count).tolist()}")
    model.seed = 11
    model.fresh_draws_per_call = True
    out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(4, 2, tol, shutter=shutters), THR, BTHR, chuncks=CHUNCKS,
                                                  lens=lens)
    torch.cuda.synchronize()
    assert model.seed == 11 + passes
    assert stats["passes"] == passes and stats["rays_rendered"] == rendered
    assert np.array_equal(stats["spp"].cpu().numpy(), want.count)
    assert A.same_bits(means_of(out).cpu().numpy(), want.mean)
    assert (want.count == 2).any() and (want.count == 4).any()


def test_the_background_cache_misses_when_only_the_lens_changes():
    from stnerf_amd.bkgd_cache import BackgroundCache
    model, K, T, ids = scene("bf16x3")
    model.set_background_cache(BackgroundCache())
    hm = lambda: (model._bkgd_cache.stats["hits"], model._bkgd_cache.stats["misses"])
    view = lambda lens, frame=ids: flat(parallel.render_view(model, K, T, H, W, frame, THR, BTHR, chuncks=CHUNCKS, lens=lens))
    a = view(Lens(*MILD))
    h0, m0 = hm()
    assert h0 == 0 and m0 > 0
    moved = [ids[0]] + [2.0 if f == 1.0 else 1.0 for f in ids[1:]]
    b = view(Lens(*MILD), moved)                                             # the same lens, the performers moved: every piece hits
    h1, m1 = hm()
    assert (h1, m1) == (m0, m0)
    view(Lens(*LC.SETS[2]), moved)                                           # only the lens changes: every piece misses
    h2, m2 = hm()
    assert (h2, m2) == (h1, 2 * m0)
    view(None, moved)                                                        # and no lens is yet another view
    h3, m3 = hm()
    assert (h3, m3) == (h2, 3 * m0)
    c = view(dict(zip(("k1", "k2", "k3", "p1", "p2"), MILD)), moved)         # back to the first lens: hits, and the hit frame's bits
    assert hm() == (h3 + m0, m3)
    assert all(torch.equal(x, y) for x, y in zip(b, c)) and not torch.equal(a[0], b[0])
    model.set_background_cache(None)
    want = view(Lens(*MILD), moved)
    assert all(torch.equal(x, y) for x, y in zip(b, want))                   # a cached lens frame is the uncached one
    torch.cuda.synchronize()


def test_the_drivers_refuse_what_a_lens_cannot_do():
    from stnerf_amd.bkgd_cache import BackgroundCache
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    pairs = list(enumerate(ids))
    deep = Lens(aperture=APERTURE, focus=FOCUS)
    with pytest.raises(ValueError, match="accumulate="):
        parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, lens=deep)
    with pytest.raises(ValueError, match="accumulate="):
        render_pose(model, T, K, H, W, pairs, 20.0, lens=deep)
    with pytest.raises(ValueError, match="too strong"):
        parallel.render_view(model, K, T, H, W, ids, THR, BTHR, chuncks=CHUNCKS, lens=Lens(k1=-3.0))
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(model, T, K, H, W, pairs, 20.0, accumulate=AccumulateSpec(2), lens=deep, scene_passes=True)
    with pytest.raises(ValueError, match="out of scope"):
        render_pose(model, T, K, H, W, pairs, 20.0, accumulate=AccumulateSpec(2), lens=deep, occluder=(torch.zeros(H, W, 4), torch.ones(H, W)))
    model.set_background_cache(BackgroundCache())
    with pytest.raises(ValueError, match="one jitter pattern"):
        parallel.render_view_accumulated(model, K, T, H, W, ids, AccumulateSpec(2), THR, BTHR, chuncks=CHUNCKS, lens=deep)
    model.set_background_cache(None)
    with pytest.raises(ValueError, match="ray window"):
        ops.generate_rays(K, T, H, W, first_ray=23, n=23, lens=Lens(*MILD))
    with pytest.raises(ValueError, match="lens_points"):
        ops.generate_rays(K, T, H, W, lens=deep)
    assert model.seed == 11
    torch.cuda.synchronize()


def test_render_pose_and_the_renderer_through_a_lens():
    from stnerf_amd.render import LayeredNeuralRenderer
    from stnerf_amd.render.render_pose import render_pose
    model, K, T, ids = scene("bf16x3")
    l, far = model.total_layers, 20.0
    pairs = list(enumerate(ids))
    lens = Lens(*MILD, aperture=APERTURE, focus=FOCUS)
    bend = Lens(*MILD)
    # render_pose, distortion only: the driver's frame with the reference's depth post-processing; scene passes come with it
    color, depth, color_layer, depth_layer = render_pose(model, T, K, H, W, pairs, far, THR, BTHR, lens=bend)
    out = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, lens=bend)
    assert same_bits(color, out[0][0].reshape(H, W, 3)) and same_bits(depth, out[0][1].reshape(H, W, 1).clamp_min(0) / far)
    assert all(same_bits(color_layer[i], out[2][i][0].reshape(H, W, 3)) for i in range(l))
    assert not same_bits(color, render_pose(model, T, K, H, W, pairs, far, THR, BTHR)[0])
    five = render_pose(model, T, K, H, W, pairs, far, THR, BTHR, lens=bend, scene_passes=True)
    with_scene = parallel.render_view(model, K, T, H, W, ids, THR, BTHR, scene=True, lens=bend)
    assert same_bits(five[0], with_scene[0][0][0].reshape(H, W, 3)) and len(five[4]["color_scene"]) == l
    assert same_bits(five[4]["color_scene"][1], with_scene[1][1][0].reshape(H, W, 3))
    # render_pose with accumulate: the accumulated driver's means
    spec = AccumulateSpec(3)
    color, depth, color_layer, depth_layer, stats = render_pose(model, T, K, H, W, pairs, far, THR, BTHR, accumulate=spec, lens=lens)
    out, flat_stats = parallel.render_view_accumulated(model, K, T, H, W, ids, spec, THR, BTHR, lens=lens)
    assert same_bits(color, out[0][0].reshape(H, W, 3)) and same_bits(depth, out[0][1].reshape(H, W, 1).clamp_min(0) / far)
    assert all(same_bits(depth_layer[i], out[2][i][1].reshape(H, W, 1) / far) for i in range(l))
    assert torch.equal(stats["spp"].reshape(-1), flat_stats["spp"]) and stats["passes"] == 3
    assert not same_bits(color, render_pose(model, T, K, H, W, pairs, far, THR, BTHR, accumulate=spec)[0])
    # the renderer over a 2-pose path: every frame is render_pose's with the stored lens; on_frame's keywords are unchanged
    K2, T2 = syn.camera(H, W, 40.0)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    poses, Ks = torch.stack([torch.as_tensor(T), torch.as_tensor(T2)]), [K, K2]
    seen = []
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=poses, gt_Ks=Ks, lens=dict(zip(("k1", "k2", "k3", "p1", "p2"), MILD)))
    r.set_path_gt_poses()
    assert isinstance(r.lens, Lens) and len(r.poses) == 2
    r.render_path(on_frame=lambda idx, c, d, cl, dl: seen.append((idx, c.clone(), d.clone())))
    assert len(seen) == 2 and len(r.images) == 2
    for k in range(2):
        c, d, _, _ = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0, lens=bend)
        assert seen[k][0] == k and same_bits(seen[k][1], c) and same_bits(seen[k][2], d)
        assert not same_bits(c, render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0)[0])
    seen.clear()
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=poses, gt_Ks=Ks, lens=lens, accumulate=dict(max_spp=2))
    r.set_path_gt_poses()
    r.render_path(on_frame=lambda idx, c, d, cl, dl, accumulated=None: seen.append((idx, c.clone(), accumulated)))
    assert len(seen) == 2 and len(r.spp_maps) == 2
    for k in range(2):
        c, _, _, _, st = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0, accumulate=r.accumulate, lens=lens)
        assert same_bits(seen[k][1], c) and seen[k][2]["passes"] == st["passes"] == 2
    # the method's own keyword wins over the stored lens
    c_none = LayeredNeuralRenderer(cfg, model=model, gt_poses=poses, gt_Ks=Ks).render_pose(poses[0], K, pairs, THR, BTHR, lens=bend)[0]
    assert same_bits(c_none, render_pose(model, T, K, H, W, pairs, far, THR, BTHR, lens=bend)[0])
    torch.cuda.synchronize()
