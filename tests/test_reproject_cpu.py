"""Reprojection of the background across nearby views, the host side (no GPU): ``ReprojectSpec``'s validation and key schedule,
plate identity, the library's argument checks and exports, and the numpy restatement (tests/reproject_common.py) against an
fp64 geometric check that shares no code with it -- on the very case set the GPU tests compare bit for bit, with the census that
keeps them from passing vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import reproject_common as R
from conftest import REPO
from stnerf_amd import hip
from stnerf_amd import reproject as rp

F = np.float32


# ---------------------------------------------------------------------------------------- spec and schedule
def test_spec_validation_and_lazy_export():
    import stnerf_amd
    assert stnerf_amd.ReprojectSpec is rp.ReprojectSpec and stnerf_amd.BackgroundPlate is rp.BackgroundPlate
    s = rp.as_spec(dict(key_every=3, rel=0.1, a_min=0.25))
    assert isinstance(s, rp.ReprojectSpec) and (s.key_every, s.rel, s.a_min) == (3, 0.1, 0.25) and rp.as_spec(s) is s
    assert "key_every=3" in repr(s)
    for bad in (dict(key_every=0), dict(key_every=2.0), dict(key_every=True), dict(rel=-0.1), dict(rel=float("nan")),
                dict(rel=float("inf")), dict(a_min=-0.1), dict(a_min=1.5), dict(a_min=float("nan"))):
        with pytest.raises(ValueError):
            rp.ReprojectSpec(**bad)
    with pytest.raises(TypeError):
        rp.as_spec(4)
    with pytest.raises(TypeError):
        rp.as_spec(dict(every=2))


@pytest.mark.parametrize("N,n_poses,want", [
    (1, 4, [(0, 1), (1, 2), (2, 3), (3,)]),
    (3, 5, [(0, 3), (0, 3), (0, 3), (3,), (3,)]),             # a path length N does not divide: the last key stands alone
    (3, 7, [(0, 3), (0, 3), (0, 3), (3, 6), (3, 6), (3, 6), (6,)]),
    (4, 3, [(0,), (0,), (0,)]),
])
def test_key_schedule(N, n_poses, want):
    s = rp.ReprojectSpec(N, 0.05, 0.5)
    assert [s.keys_of(i, n_poses) for i in range(n_poses)] == want
    for i in (-1, n_poses):
        with pytest.raises(ValueError):
            s.keys_of(i, n_poses)


def test_plate_rows_are_straight_colour_alpha_and_expected_depth():
    mixed = torch.tensor([[0.2, 0.4, 0.1, 2.0, 0.5], [0.1, 0.1, 0.1, 0.3, 0.1], [0.0, 0.0, 0.0, 0.0, 0.0],
                          [0.3, 0.3, 0.3, 1.0, float("nan")]])
    rows = rp.plate_rows(mixed, 0.25)
    assert torch.equal(rows[0], torch.tensor([0.2 / 0.5, 0.4 / 0.5, 0.1 / 0.5, 0.5, 2.0 / 0.5]))
    for i in (1, 2, 3):                                      # below a_min, empty, NaN: absent
        assert torch.equal(rows[i, :4], torch.zeros(4)) and bool(torch.isnan(rows[i, 4]))
    assert rows.is_contiguous() and rp.plate_rows(mixed, 0.0)[1, 3] == 0.1


# ---------------------------------------------------------------------------------------- plate identity
def _model():
    from instances_common import base_model
    m = base_model(2)
    m.seed, m.fresh_draws_per_call = 11, False
    return m


def test_plate_identity_equality_and_inequality():
    m = _model()
    ids = [1.0, 2.5, 3.0]
    ident = lambda **kw: rp.background_identity(m, kw.get("ids", ids), 17, 23, kw.get("chuncks", 3584), kw.get("thr", 0.0), kw.get("bthr", 0.0))
    base = ident()
    assert base == ident() and hash(base) == hash(ident())
    # what acts on other layers leaves it alone: performer frame ids, a performer's shift; and, for a time-independent
    # background, layer 0's own frame id
    assert base == ident(ids=[1.0, 1.0, 2.0]) == ident(ids=[2.0, 2.5, 3.0])
    m.shift = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.0]]
    shifted = ident()                                        # (a shift list names layer 0's shift too, if only as zeros)
    m.shift = [[0.0, 0.0, 0.0], [0.0, 0.3, 0.0], [0.2, 0.0, 0.0]]
    assert shifted == ident()
    m.shift = None
    # a small view renders with the model's default thresholds whatever the call's are; a large one with the call's
    assert base == ident(thr=0.3, bthr=0.2)
    assert ident(chuncks=64) != base and ident(chuncks=64, bthr=0.2) != ident(chuncks=64) and ident(chuncks=64, bthr=0.2) == ident(chuncks=64, bthr=0.2)
    # what layer 0 depends on changes it: its shift, its opacity entry, the seed, the precision, its weights, the sample counts
    m.shift = [[0.1, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    assert ident() != base
    m.shift = None
    assert ident() == base
    m.layer_alpha = [0.5, 1.0, 1.0]
    assert ident() != base
    m.layer_alpha = [1.0, 0.5, 1.0]
    with_table = ident()
    m.layer_alpha = [1.0, 0.25, 0.7]
    assert ident() == with_table                             # (a performer's opacity is not the background's)
    m.layer_alpha = None
    m.seed = 12
    assert ident() != base
    m.seed = 11
    m.set_precision("fp32")
    assert ident() != base
    m.set_precision("bf16x3")
    assert ident() == base
    m.fine_ray_sample += 1
    assert ident() != base
    m.fine_ray_sample -= 1
    with torch.no_grad():
        next(m.bkgd_spacenet.parameters()).add_(1.0)
    assert ident() != base
    # a time-dependent background: layer 0's frame id joins
    m2 = _model()
    m2.bkgd_use_space_time = True                            # (with USE_SPACE_TIME, which the synthetic model has)
    a = rp.background_identity(m2, [1.0, 2.5, 3.0], 17, 23, 3584, 0.0, 0.0)
    assert a != rp.background_identity(m2, [2.0, 2.5, 3.0], 17, 23, 3584, 0.0, 0.0) and a == rp.background_identity(m2, [1.0, 1.0, 1.0], 17, 23, 3584, 0.0, 0.0)


def test_a_plate_keeps_its_camera_and_depth_column():
    rows = torch.rand(6, 5)
    K, T = R.camera(2, 3, 7.0)
    p = rp.BackgroundPlate(K, T, 2, 3, rows, ("id",), index=4)
    assert torch.equal(p.t, rows[:, 4]) and p.t.is_contiguous() and p.index == 4 and p.identity == ("id",)
    assert p.source()[2:4] == (2, 3) and p.source()[4] is rows and torch.equal(p.K, torch.from_numpy(K))
    with pytest.raises(ValueError):
        rp.BackgroundPlate(K, T, 2, 3, torch.rand(5, 5), None)


# ---------------------------------------------------------------------------------------- the restatement against fp64 geometry
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_agrees_with_fp64_geometry(name):
    srcs, (K_d, T_d, h_d, w_d), rel = R.build_case(name)
    r = R.oracle_case(name)
    worst_px, worst_t = R.geometry_errors(r, [(s[0], s[2], s[4], s[6]) for s in srcs], K_d, T_d, w_d)
    print(name, R.census(r), "worst |du|,|dv|", worst_px, "worst rel t'", worst_t)
    assert worst_px <= 0.5 + R.PIXEL_SLACK and worst_t <= R.T_REL
    # the hole list is the ascending list of src < 0, and filled + holes = the view
    assert r["n_holes"] + int((r["src"] >= 0).sum()) == h_d * w_d and np.array_equal(r["holes"], np.flatnonzero(r["src"] < 0))
    assert (np.diff(r["holes"]) > 0).all() and np.isnan(r["t"][r["holes"]]).all() and not r["values"][r["holes"]].any()
    assert np.array_equal(r["empty"] | r["guard"], r["src"] < 0) and not (r["empty"] & r["guard"]).any()


def test_the_case_set_exercises_every_rule():
    """What the GPU tests compare bit for bit holds an empty-key hole, a guard hole, a collision won by depth and an exact tie
    won by id -- asserted on the oracle's output, so a GPU test cannot pass without the kernels having met them."""
    census = {name: R.census(R.oracle_case(name)) for name in R.CASES}
    for name, c in sorted(census.items()):
        print(name, c)
    assert census["orbit_3"]["empty"] > 0 and census["orbit_3"]["guard"] > 0 and census["orbit_3"]["depth"] > 0
    assert census["orbit_15"]["empty"] > census["orbit_3"]["empty"] and census["orbit_15"]["depth"] > 0
    assert census["dist_4_to_3"]["empty"] > 0 and census["dist_4_to_3"]["guard"] > 0          # magnification: cracks
    assert census["two_sources"]["depth"] > 0 and census["two_sources"]["empty"] < census["orbit_3"]["empty"]
    assert census["tie_twice"]["tie"] == census["tie_twice"]["filled"] + census["tie_twice"]["guard"] > 0
    tie = R.oracle_case("tie_twice")
    assert (tie["src"][tie["src"] >= 0] < R.H * R.W).all()                                     # the lower id won every tie
    same = R.oracle_case("same_camera")
    assert same["n_holes"] == 0 and np.array_equal(same["src"], np.arange(R.H * R.W))
    assert census["truncated_1"]["filled"] == 0 and 0 < census["truncated_63"]["filled"] < census["truncated_65"]["filled"]
    # every filled pixel of every case has a source in the first id range unless a second source was given
    for name in R.CASES:
        n_src = sum(len(s[6]) for s in R.build_case(name)[0])
        assert R.oracle_case(name)["src"].max() < n_src


def test_absent_rows_and_points_behind_the_camera_reach_nothing():
    K, T = R.camera(R.H, R.W)
    t, values = R.analytic_frame(K, T, R.H, R.W)
    K_d, T_d = R.camera(R.H, R.W, 3.0)
    Wd, o_d = R.world_to_camera(T_d), T_d[:3, 3]
    bad = t.copy()
    bad[::3] = np.nan
    bad[1::3] = 0.0
    bad[2::3] = -1.0
    assert len(R.splat_rows(R.kinv_of(K), T, R.W, bad, 0, K_d, Wd, o_d, R.H, R.W)[0]) == 0
    bad[5] = np.inf
    assert len(R.splat_rows(R.kinv_of(K), T, R.W, bad, 0, K_d, Wd, o_d, R.H, R.W)[0]) == 0
    K_b, T_b = R.camera(R.H, R.W, 0.0, -8.0)                 # at z = +8, beyond the far plane, looking away from it: every point is behind
    assert len(R.splat_rows(R.kinv_of(K), T, R.W, t, 0, K_b, R.world_to_camera(T_b), T_b[:3, 3], R.H, R.W)[0]) == 0
    K_o, T_o = R.camera(R.H, R.W, 80.0)                      # from the side: part of the far plane leaves the image
    assert 0 < len(R.splat_rows(R.kinv_of(K), T, R.W, t, 0, K_o, R.world_to_camera(T_o), T_o[:3, 3], R.H, R.W)[0]) < R.H * R.W


# ---------------------------------------------------------------------------------------- the C ABI
NEW = ("stnerf_reproject_splat", "stnerf_reproject_resolve", "stnerf_reproject_holes", "stnerf_reproject_holes_workspace_bytes")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "stnerf.h")).read()
    declared = set(re.findall(r"\b(stnerf_[a-z_0-9]+)\s*\(", header))
    assert set(NEW) <= declared and set(NEW) <= set(hip.exported_symbols())
    assert "#define STNERF_REPROJECT_MAX_SOURCES 4" in header and hip.REPROJECT_MAX_SOURCES == 4
    assert C.sizeof(hip.ReprojectSource) == 24
    lib = hip.lib()
    for name in NEW:
        assert getattr(lib, name) is not None
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True)
    if out.returncode == 0:                                  # (the export list itself, where binutils is there)
        exported = set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
        assert set(NEW) <= exported


def _f(*v):
    return (C.c_float * len(v))(*v)


def test_argument_errors_before_any_launch():
    """Every EINVAL of include/stnerf.h, with pointers that are never dereferenced (no GPU here: a launch would fail otherwise)."""
    lib = hip.lib()
    fake = C.c_void_p(1 << 20)
    null = C.c_void_p(0)
    k9, t16, w12, o3 = _f(*([1.0] * 9)), _f(*([1.0] * 16)), _f(*([1.0] * 12)), _f(0.0, 0.0, 0.0)

    def splat(kinv=k9, T=t16, h_s=17, w_s=23, t=fake, n=391, base=0, K=k9, W=w12, o=o3, h_d=17, w_d=23, z=1e-6, keys=fake):
        return lib.stnerf_reproject_splat(kinv, T, h_s, w_s, t, n, base, K, W, o, h_d, w_d, z, keys, None)
    for kw in (dict(kinv=None), dict(T=None), dict(t=null), dict(K=None), dict(W=None), dict(o=None), dict(keys=null),
               dict(h_s=0), dict(w_s=0), dict(h_s=1 << 16, w_s=1 << 16), dict(h_d=0), dict(w_d=-1), dict(h_d=1 << 16, w_d=1 << 15),
               dict(n=-1), dict(n=392), dict(base=-1), dict(base=(1 << 31) - 390), dict(z=-1e-6), dict(z=float("nan")), dict(z=float("inf"))):
        assert splat(**kw) == hip.EINVAL, kw
        assert "reproject_splat" in hip.last_error()
    assert splat(n=0) == hip.OK and splat(n=0, base=1 << 31) == hip.OK          # nothing to do: no launch

    def table(*recs):
        arr = (hip.ReprojectSource * max(len(recs), 1))()
        for i, (v, stride, n) in enumerate(recs):
            arr[i].values, arr[i].row_stride, arr[i].n = v, stride, n
        return arr
    one = table((fake.value, 5, 391))

    def resolve(keys=fake, h=17, w=23, rel=0.05, tab=one, ns=1, Cn=5, v=fake, t=fake, s=fake):
        return lib.stnerf_reproject_resolve(keys, h, w, rel, tab, ns, Cn, v, t, s, None)
    five = table(*[(fake.value, 5, 10)] * 5)
    for kw in (dict(keys=null), dict(tab=None), dict(v=null), dict(t=null), dict(s=null), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15),
               dict(Cn=0), dict(Cn=65), dict(rel=-0.01), dict(rel=float("nan")), dict(ns=0), dict(ns=5, tab=five),
               dict(tab=table((fake.value, 4, 391))), dict(tab=table((fake.value, 5, -1))), dict(tab=table((0, 5, 391))),
               dict(ns=2, tab=table((fake.value, 5, (1 << 31) - 1), (fake.value, 5, 1)))):
        assert resolve(**kw) == hip.EINVAL, kw
        assert "reproject_resolve" in hip.last_error()
    assert "row stride" in (resolve(tab=table((fake.value, 4, 391))), hip.last_error())[1]

    assert lib.stnerf_reproject_holes_workspace_bytes(0) == hip.EINVAL and lib.stnerf_reproject_holes_workspace_bytes(1 << 31) == hip.EINVAL
    need = lib.stnerf_reproject_holes_workspace_bytes(391)
    assert need == 256 and lib.stnerf_reproject_holes_workspace_bytes(256 * 64 + 1) == 512
    assert need == lib.stnerf_accumulate_select_workspace_bytes(391)
    for args in ((null, 391, fake, fake, fake, need), (fake, 391, null, fake, fake, need), (fake, 391, fake, null, fake, need),
                 (fake, 391, fake, fake, null, need), (fake, 0, fake, fake, fake, need), (fake, 1 << 31, fake, fake, fake, 1 << 40),
                 (fake, 391, fake, fake, fake, need - 1)):
        assert lib.stnerf_reproject_holes(*args, None) == hip.EINVAL, args
        assert "reproject_holes" in hip.last_error()
