"""The lens model in ray generation, the host side (no GPU): the schedule of lens points, what the oracle's rays
(tests/lens_common.py) MEAN -- distortion against the fp64 Brown-Conrady forward model, defocus against the plane in focus --, the
walk over the table, ``Lens``'s validation and ``Lens.check``, the drivers' refusals on a stub model, the view key, and the
library's argument checks."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import lens_common as LC
from stnerf_amd import hip, lens as L, parallel
from stnerf_amd.accumulate import AccumulateSpec

F = np.float32
H1080, W1080, FOCAL = 1080, 1920, 1500.0


# ---------------------------------------------------------------------------------------- schedule
def test_pass_zero_is_the_lens_centre_and_every_point_is_inside_the_disk():
    assert L.lens_point(0) == (0.0, 0.0)
    for p in range(1024):
        x, y = L.lens_point(p)
        assert isinstance(x, float) and float(F(x)) == x and float(F(y)) == y
        assert x * x + y * y <= 1.0, (p, x, y)
        assert (x, y) == tuple(float(c) for c in LC.lens_point(p)), p
    import stnerf_amd
    assert stnerf_amd.Lens is L.Lens
    lens = L.Lens(aperture=0.25, focus=3.0)
    tab = lens.table(16)
    assert tab.dtype == F and tab.shape == (16, 2) and LC.same_bits(tab, LC.table(16, 0.25)) and not tab[0].any()
    assert all(tab[p, 0] == F(0.25 * L.lens_point(p)[0]) for p in range(16))
    with pytest.raises(ValueError):
        lens.table(0)
    with pytest.raises(ValueError):
        L.lens_point(-1)


def _cells(n):
    """Counts of the first n points in quadrant x equal-area ring (r^2 < 1/2 | r^2 >= 1/2); the centre counts as x >= 0, y >= 0."""
    counts = np.zeros((4, 2), int)
    for p in range(n):
        x, y = L.lens_point(p)
        counts[(0 if x >= 0 else 1) + (0 if y >= 0 else 2), int(x * x + y * y >= 0.5)] += 1
    return counts


def test_every_prefix_is_spread_over_the_disk():
    eight = _cells(8)
    print("8 passes, per quadrant:", eight.sum(1).tolist())
    assert eight.sum(1).tolist() == [2, 2, 2, 2]
    cells = _cells(64)
    print("64 passes, quadrant x ring:", cells.tolist(), "max / share =", cells.max() / 8.0)
    assert cells.min() >= 1 and cells.max() <= 1.5 * 8


# ---------------------------------------------------------------------------------------- what the rays mean
GRID = np.array([[int(round(j * (W1080 - 1) / 96.0)), int(round(i * (H1080 - 1) / 54.0))] for i in range(55) for j in range(97)])


@pytest.mark.parametrize("coeffs", LC.SETS)
def test_distorted_rays_return_to_their_pixel_through_the_fp64_forward_model(coeffs):
    """The oracle's fp32 ray of a pixel, as normalised coordinates x = d_x / d_z, pushed through the fp64 forward model and K, lands
    on the pixel within 1e-3 px: eight times the fp32 floor of the 20-round inverse (1.3e-4 px at f = 1500 over 1080p).  A wrong sign
    or a swapped p1 / p2 misses by whole pixels."""
    K, kinv = LC.intrinsics(FOCAL, H1080, W1080)
    pix = GRID[:, 1] * W1080 + GRID[:, 0]
    rays = LC.rays_of_lens(kinv, np.eye(4, dtype=F), W1080, pix, coeffs=coeffs).astype(np.float64)
    x, y = rays[:, 3] / rays[:, 5], rays[:, 4] / rays[:, 5]
    xd, yd = LC.forward64(x, y, *coeffs)
    Kd = K.numpy().astype(np.float64)
    u, v = xd * Kd[0, 0] + Kd[0, 2], yd * Kd[1, 1] + Kd[1, 2]
    err = np.maximum(np.abs(u - GRID[:, 0]), np.abs(v - GRID[:, 1]))
    moved = np.hypot(x * Kd[0, 0] + Kd[0, 2] - GRID[:, 0], y * Kd[1, 1] + Kd[1, 2] - GRID[:, 1])
    print(f"{coeffs}: max round-trip residual {err.max():.3e} px; the lens moves a ray by up to {moved.max():.1f} px")
    assert err.max() <= 1e-3
    assert moved.max() > 10.0                                                 # not vacuous: tens of pixels at the corners
    # a swapped p1 / p2 or a wrong sign of k1 is told apart by whole pixels
    if coeffs[3] != coeffs[4]:
        sx, sy = LC.forward64(x, y, coeffs[0], coeffs[1], coeffs[2], coeffs[4], coeffs[3])
        assert np.abs(sx * Kd[0, 0] + Kd[0, 2] - GRID[:, 0]).max() > 1.0
    wx, _ = LC.forward64(x, y, -coeffs[0], *coeffs[1:])
    assert np.abs(wx * Kd[0, 0] + Kd[0, 2] - GRID[:, 0]).max() > 1.0
    # and the package's own fp64 statement of the iteration and of the forward model agree with the oracle's
    lens = L.Lens(*coeffs)
    cam = np.stack([GRID[:, 0], GRID[:, 1], np.ones(len(GRID))], 1) @ kinv.astype(np.float64).T
    ux, uy = lens.undistort(cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2])
    assert np.abs(ux - x).max() <= 1e-6 and np.abs(uy - y).max() <= 1e-6
    fx, fy = L.forward_distortion(ux, uy, *coeffs)
    gx, gy = LC.forward64(ux, uy, *coeffs)
    assert np.abs(fx - gx).max() <= 1e-12 and np.abs(fy - gy).max() <= 1e-12
    lens.check(K, H1080, W1080)


def _pose():
    a = np.deg2rad(25.0)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s, -4.0 * s], [0.0, 1.0, 0.0, 0.3], [-s, 0.0, c, -4.0 * c], [0.0, 0.0, 0.0, 1.0]], F)


@pytest.mark.parametrize("distorted", [False, True])
def test_every_lens_point_sends_the_ray_through_the_pinhole_point_on_the_plane_in_focus(distorted):
    """For every point of an 8-point table: the oracle's ray, evaluated in fp64 at camera depth ``focus``, hits the pinhole ray's point
    on that plane within 0.01 aperture (aperture = 0.05 focus; fp32 rounding is about 1e-6 focus = 2e-5 aperture, a wrong sign misses
    by 2 aperture), and its origin lies at aperture |point| from the pinhole under the same bound."""
    focus = 3.0
    aperture = 0.05 * focus
    K, kinv = LC.intrinsics(FOCAL, H1080, W1080)
    T = _pose()
    T64 = T.astype(np.float64)
    coeffs = LC.SETS[1] if distorted else None
    pix = (GRID[:, 1] * W1080 + GRID[:, 0])[::7]
    tab = LC.table(8, aperture)
    pin = LC.rays_of_lens(kinv, T, W1080, pix, coeffs=coeffs).astype(np.float64)
    axis = T64[:3, 2]                                                       # the optical axis in world coordinates
    t_pin = focus / (pin[:, 3:6] @ axis)
    target = pin[:, 0:3] + pin[:, 3:6] * t_pin[:, None]
    worst_hit = worst_origin = 0.0
    for p in range(8):
        rays = LC.rays_of_lens(kinv, T, W1080, pix, coeffs=coeffs, points=tab, phase=p, focus=focus).astype(np.float64)
        depth0 = (rays[:, 0:3] - T64[:3, 3]) @ axis                          # the origin lies in the lens plane: camera z = 0
        t = (focus - depth0) / (rays[:, 3:6] @ axis)
        hit = rays[:, 0:3] + rays[:, 3:6] * t[:, None]
        worst_hit = max(worst_hit, float(np.linalg.norm(hit - target, axis=1).max()))
        off = np.linalg.norm(rays[:, 0:3] - pin[:, 0:3], axis=1)
        worst_origin = max(worst_origin, float(np.abs(off - float(np.hypot(*tab[p].astype(np.float64)))).max()))
        assert np.abs(depth0).max() <= 0.01 * aperture
        if p == 0:
            assert LC.same_bits(rays.astype(F), pin.astype(F))               # the lens centre: the pinhole ray, bit for bit
        else:
            assert off.min() > 0.1 * aperture
    print(f"distorted={distorted}: worst miss on the plane {worst_hit / aperture:.2e} aperture, worst origin error {worst_origin / aperture:.2e} aperture")
    assert worst_hit <= 0.01 * aperture and worst_origin <= 0.01 * aperture
    # a wrong sign of the lens point in the direction misses by 2 aperture |point|
    flipped = pin[:, 0:3] + 2 * (rays[:, 0:3] - pin[:, 0:3])
    assert np.linalg.norm(flipped - pin[:, 0:3], axis=1).min() > 0.5 * aperture


# ---------------------------------------------------------------------------------------- the walk
def test_the_walk_over_the_table():
    h, w, M = 17, 23, 8
    pix = np.arange(h * w)
    for p in range(M):
        assert (LC.table_rows(pix, M, p, False) == p).all()
    for key in (0, 0x9E3779B9):
        rows = np.stack([LC.table_rows(pix, M, p, True, key) for p in range(M)])
        assert (np.sort(rows, 0) == np.arange(M)[:, None]).all()              # every pixel: each row exactly once
        assert len(np.unique(rows[0])) == M                                  # and the pixels start in different places
    assert not np.array_equal(LC.table_rows(pix, M, 0, True, 0), LC.table_rows(pix, M, 0, True, 0x9E3779B9))
    # the mixer by hand on two words
    assert int(LC.lens_hash(np.uint32(0))) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(LC.lens_hash(np.uint32(1))) == x
    # through the oracle's rays: without decorrelate every origin of pass p is the pinhole's moved by row p
    _, kinv = LC.intrinsics(30.0, h, w)
    tab = LC.table(M, 0.2)
    T = np.eye(4, dtype=F)
    for p in (1, 5):
        rays = LC.rays_of_lens(kinv, T, w, pix, points=tab, phase=p, focus=2.0)
        assert (rays[:, 0] == tab[p, 0]).all() and (rays[:, 1] == tab[p, 1]).all() and not rays[:, 2].any()
        rays = LC.rays_of_lens(kinv, T, w, pix, points=tab, phase=p, decorrelate=True, key=3, focus=2.0)
        assert LC.same_bits(rays[:, 0:2], tab[LC.table_rows(pix, M, p, True, 3)])


# ---------------------------------------------------------------------------------------- Lens
def test_lens_defaults_validation_and_check():
    lens = L.Lens()
    assert (lens.coefficients, lens.aperture, lens.focus, lens.decorrelate, lens.key) == ((0.0,) * 5, 0.0, None, True, 0)
    assert not lens.enabled and not lens.distorts
    assert L.Lens(k1=-0.1).enabled and L.Lens(k1=-0.1).distorts and L.Lens(p2=1e-3).distorts
    assert L.Lens(aperture=0.1, focus=2.0).enabled and not L.Lens(aperture=0.1, focus=2.0).distorts and not L.Lens(focus=2.0).enabled
    assert L.as_lens(None) is None and L.as_lens(lens) is lens and L.as_lens(dict(k1=0.2, key=7)).fingerprint() == L.Lens(k1=0.2, key=7).fingerprint()
    with pytest.raises(TypeError):
        L.as_lens(0.1)
    for bad in (dict(k1=float("nan")), dict(p2=float("inf")), dict(k3=1e40), dict(aperture=-0.1), dict(aperture=float("nan")),
                dict(aperture=0.1), dict(aperture=0.1, focus=0.0), dict(aperture=0.1, focus=-2.0), dict(focus=float("inf")),
                dict(aperture=0.1, focus=float("nan")), dict(key=-1), dict(key=1 << 32), dict(key=0.5)):
        with pytest.raises(ValueError):
            L.Lens(**bad)
    # the fingerprint holds every field
    base = dict(k1=-0.1, k2=0.02, k3=0.001, p1=0.001, p2=-0.0005, aperture=0.1, focus=2.0, decorrelate=True, key=1)
    prints = {L.Lens(**base).fingerprint()}
    for name, other in (("k1", -0.2), ("k2", 0.03), ("k3", 0.0), ("p1", 0.0), ("p2", 0.0), ("aperture", 0.2), ("focus", 3.0),
                        ("decorrelate", False), ("key", 2)):
        prints.add(L.Lens(**dict(base, **{name: other})).fingerprint())
    assert len(prints) == 10 and all(isinstance(hash(p), int) for p in prints)
    # check: the four sets pass at f = 1500 over 1080p; a strong lens at a wide view is refused; so is a K^-1 with a tilted third row
    K, _ = LC.intrinsics(FOCAL, H1080, W1080)
    for coeffs in LC.SETS:
        L.Lens(*coeffs).check(K, H1080, W1080)
    wide, _ = LC.intrinsics(400.0, H1080, W1080)
    with pytest.raises(ValueError, match="too strong"):
        L.Lens(*LC.SETS[3]).check(wide, H1080, W1080)
    with pytest.raises(ValueError, match="too strong"):
        L.Lens(k1=-1.0).check(K, H1080, W1080)
    L.Lens(aperture=0.1, focus=2.0).check(wide, H1080, W1080)                # no distortion: nothing to converge
    tilted = K.clone()
    tilted[2, 0] = 1e-4
    for lens in (L.Lens(k1=-0.1), L.Lens(aperture=0.1, focus=2.0)):
        with pytest.raises(ValueError, match="third row"):
            lens.check(tilted, H1080, W1080)


# ---------------------------------------------------------------------------------------- the drivers' refusals
def _fake_model(**over):
    m = types.SimpleNamespace(total_layers=3, layer_num=2, seed=5, fresh_draws_per_call=True, replay=None, ray_window=(0, 0, 0),
                              _bkgd_cache=None, _layer_cache=None, _occupancy=None, shard_views=False)
    for k, v in over.items():
        setattr(m, k, v)
    return m


K4, T4 = torch.tensor([[8.0, 0.0, 2.0], [0.0, 8.0, 2.0], [0.0, 0.0, 1.0]]), torch.eye(4)
IDS = [1.0, 2.0, 3.0]


def test_the_drivers_name_what_they_refuse(monkeypatch):
    """Every refusal is raised before anything touches the device (there is none here) and leaves the seed alone."""
    from stnerf_amd import ops
    from stnerf_amd.render.render_pose import render_pose
    view = lambda model, **kw: parallel.render_view(model, K4, T4, 4, 4, IDS, device="cpu", **kw)
    accu = lambda model, lens, spec=AccumulateSpec(2), **kw: parallel.render_view_accumulated(model, K4, T4, 4, 4, IDS, spec, device="cpu",
                                                                                            lens=lens, **kw)
    m = _fake_model()
    with pytest.raises(ValueError, match="accumulate="):                      # defocus needs several passes
        view(m, lens=L.Lens(aperture=0.1, focus=2.0))
    with pytest.raises(ValueError, match="accumulate="):
        view(m, lens=dict(k1=-0.1, aperture=0.1, focus=2.0))
    with pytest.raises(ValueError, match="accumulate="):
        render_pose(m, T4, K4, 4, 4, list(enumerate(IDS)), 20.0, lens=L.Lens(aperture=0.1, focus=2.0), device="cpu")
    with pytest.raises(TypeError):
        view(m, lens=0.5)
    with pytest.raises(ValueError, match="too strong"):                       # Lens.check, by both drivers
        view(m, lens=L.Lens(k1=-30.0))
    with pytest.raises(ValueError, match="too strong"):
        accu(m, L.Lens(k1=-30.0))
    tilted = K4.clone()
    tilted[2, 1] = 0.01
    with pytest.raises(ValueError, match="third row"):
        parallel.render_view(m, tilted, T4, 4, 4, IDS, device="cpu", lens=L.Lens(k1=-0.1))
    # the accumulated driver's own refusals stand with a lens
    lens = L.Lens(k1=-0.1, aperture=0.1, focus=2.0)
    with pytest.raises(ValueError, match="out of scope"):
        accu(m, lens, scene=True)
    with pytest.raises(ValueError, match="out of scope"):
        accu(m, lens, occluder=torch.zeros(16, 5))
    with pytest.raises(ValueError, match="one jitter pattern"):
        accu(_fake_model(_bkgd_cache=object()), lens)
    with pytest.raises(ValueError, match="replay"):
        accu(_fake_model(replay={"jitter": None}), lens)
    assert m.seed == 5
    # ops: no ray window with an enabled lens; a table is needed with an aperture; a disabled lens is no lens
    with pytest.raises(ValueError, match="ray window"):
        ops.generate_rays(K4, T4, 4, 4, first_ray=4, lens=L.Lens(k1=-0.1), device="cpu")
    with pytest.raises(ValueError, match="ray window"):
        ops.generate_rays(K4, T4, 4, 4, stripe=4, period=8, lens=dict(aperture=0.1, focus=2.0), device="cpu")
    with pytest.raises(ValueError, match="lens_points"):
        ops.generate_rays(K4, T4, 4, 4, lens=L.Lens(aperture=0.1, focus=2.0), device="cpu")
    with pytest.raises(ValueError, match="lens_points"):
        ops.generate_rays(K4, T4, 4, 4, lens=L.Lens(aperture=0.1, focus=2.0), lens_points=torch.zeros(4, 3), device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.generate_rays(K4, T4, 4, 4, lens=L.Lens(aperture=0.1, focus=2.0), lens_points=torch.zeros(4, 2), device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.generate_rays(K4, T4, 4, 4, lens=L.Lens(k1=-0.1), device="cpu")
    # a sharded view
    monkeypatch.setattr(parallel, "active_group", lambda model=None: (0, 2, None))
    with pytest.raises(RuntimeError, match="one rank"):
        parallel.render_view(_fake_model(shard_views=True), K4, T4, 4, 4, IDS, chuncks=8, device="cpu", lens=L.Lens(k1=-0.1))
    with pytest.raises(RuntimeError, match="one rank"):
        accu(_fake_model(shard_views=True), lens)


def test_the_renderer_stores_the_lens():
    from stnerf_amd.render import LayeredNeuralRenderer
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[4, 4]), OUTPUT_DIR="")
    make = lambda **kw: LayeredNeuralRenderer(cfg, model=_fake_model(), gt_poses=T4[None], gt_Ks=[K4], **kw)
    assert make().lens is None
    r = make(lens=dict(k1=-0.1, aperture=0.1, focus=2.0))
    assert isinstance(r.lens, L.Lens) and r.lens.fingerprint() == L.Lens(k1=-0.1, aperture=0.1, focus=2.0).fingerprint()
    lens = L.Lens(k2=0.01)
    assert make(lens=lens).lens is lens
    with pytest.raises(TypeError):
        make(lens=3)
    with pytest.raises(ValueError, match="accumulate="):                      # the stored lens reaches render_pose
        r.render_pose(T4, K4, list(enumerate(IDS)))


def test_the_lens_joins_the_view_key():
    cached = _fake_model(_bkgd_cache=object())
    key = lambda lens: parallel._view_key(cached, K4, T4, 4, 4, IDS, lens)
    plain = parallel._view_key(cached, K4, T4, 4, 4, IDS)
    assert key(None) == plain and key(L.Lens()) == plain                      # no lens, a disabled lens: today's key
    a, b = key(L.Lens(k1=-0.1)), key(L.Lens(k1=-0.2))
    assert a != plain and a != b and a == key(L.Lens(k1=-0.1)) and a[1] == plain[1] and hash(a) != hash(plain)
    assert key(L.Lens(k1=-0.1, key=1)) != a
    assert parallel._view_key(_fake_model(), K4, T4, 4, 4, IDS, L.Lens(k1=-0.1)) is None      # no cache: no key, no cost


# ---------------------------------------------------------------------------------------- the library's host checks
def test_the_record_matches_the_header(tmp_path):
    import os
    import shutil
    import subprocess
    assert C.sizeof(hip.LensRecord) == 56 and hip.LensRecord().struct_size == 56
    gcc = shutil.which("gcc")
    if gcc is None:
        return
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(stnerf_lens));', 'printf("iters %d\\n", STNERF_LENS_ITERS);']
    lines += [f'printf("{name} %zu\\n", offsetof(stnerf_lens, {name}));' for name, _ in hip.LensRecord._fields_]
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(tmp_path / "layout")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(hip.LensRecord) and int(got["iters"]) == L.ITERS == LC.ITERS
    for name, _ in hip.LensRecord._fields_:
        assert int(got[name]) == getattr(hip.LensRecord, name).offset, name


def test_the_entry_checks_its_arguments_before_any_launch():
    lib = hip.lib()
    fake, null = C.c_void_p(1 << 20), C.c_void_p(0)           # (never dereferenced)
    kin = (C.c_float * 9)(0.125, 0, -0.25, 0, 0.125, -0.25, 0, 0, 1)
    tin, fin = (C.c_float * 16)(), (C.c_float * 3)()

    def gen(rec, h=4, w=4, n=4, du=0.0, dv=0.0, cols=3, stride=9, rays=fake, k=kin):
        return lib.stnerf_generate_rays_lens(k, tin, h, w, null, n, du, dv, None if rec is None else C.byref(rec), fin, cols, rays, stride, None)

    distort = lambda **kw: hip.LensRecord(**dict(dict(distort=1, k1=-0.1), **kw))
    thin = lambda **kw: hip.LensRecord(**dict(dict(points=fake.value, n_points=4, phase=1, focus=2.0), **kw))
    for rec in (None, hip.LensRecord(), distort(), thin(), distort(points=fake.value, n_points=1, focus=1.0)):
        assert gen(rec, n=0) == hip.OK                                                 # nothing to do: no launch
        # everything the pixel-list entry refuses, with and without a lens
        for bad in (gen(rec, n=17), gen(rec, n=-1), gen(rec, h=0), gen(rec, w=0), gen(rec, h=1 << 16, w=1 << 16), gen(rec, du=float("nan")),
                    gen(rec, dv=float("nan")), gen(rec, cols=18), gen(rec, stride=8), gen(rec, rays=null), gen(rec, k=None)):
            assert bad == hip.EINVAL
    assert gen(distort(), n=17) == hip.EINVAL and "at most once" in hip.last_error()
    # the record's size comes first: even a disabled record, even with n = 0
    for rec in (hip.LensRecord(), distort(), thin()):
        rec.struct_size = 52
        assert gen(rec, n=0) == hip.EINVAL and "struct_size" in hip.last_error()
    # coefficients
    for name in ("k1", "k2", "k3", "p1", "p2"):
        for value in (float("nan"), float("inf"), float("-inf")):
            assert gen(distort(**{name: value})) == hip.EINVAL and "coefficient" in hip.last_error()
    # the third row of K^-1
    for row in ((1e-3, 0, 1), (0, 1e-3, 1), (0, 0, 0), (0, 0, float("nan")), (0, 0, float("inf"))):
        tilted = (C.c_float * 9)(0.125, 0, -0.25, 0, 0.125, -0.25, *row)
        for rec in (distort(), thin()):
            assert gen(rec, k=tilted) == hip.EINVAL and "third row" in hip.last_error()
        assert gen(hip.LensRecord(), n=0, k=tilted) == hip.OK                          # no lens: the pixel-list entry takes any K^-1
    # the table
    for rec in (thin(n_points=0), thin(n_points=-3), thin(phase=-1), thin(phase=4), thin(focus=0.0), thin(focus=-2.0),
                thin(focus=float("nan")), thin(focus=float("inf"))):
        assert gen(rec) == hip.EINVAL
    assert gen(thin(phase=4)) == hip.EINVAL and "phase" in hip.last_error()
    assert gen(thin(focus=-2.0)) == hip.EINVAL and "focus" in hip.last_error()
    mirrored = (C.c_float * 9)(0.125, 0, -0.25, 0, 0.125, -0.25, 0, 0, -1)              # k < 0: the plane in focus lies at negative z
    assert gen(thin(focus=-2.0), n=0, k=mirrored) == hip.OK and gen(thin(focus=2.0), n=0, k=mirrored) == hip.EINVAL
    # without points the table's fields are not read
    assert gen(distort(n_points=-1, phase=9, focus=float("nan")), n=0) == hip.OK
