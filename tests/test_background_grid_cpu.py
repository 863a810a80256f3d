"""The background's occupancy grid without a GPU (include/stnerf.h: "Background sample cull"): the numpy
restatement of the rule on hand-made points; the ``OccupancyGrids`` background API (keys, the refusals that stay, the fingerprint,
the background cache's key); the entries' argument checks that need no device; and the two conditions of every oracle-compared
case of tests/test_gpu_background_grid.py, asserted here on the CPU oracle alone: at most 5 % of the rays left out (a background
point within eps = 5.5e-5 of an interior cell face), at least 8 rays with both listed and skipped background samples per stage."""
import ctypes as C

import numpy as np
import pytest
import torch

import background_grid_common as BG
import occupancy_common as OC
import sample_cull_common as SC
import scene_edits_common as S
from stnerf_amd import hip, occupancy as occ
from test_bkgd_cache_cpu import key_of, make_model

INF = np.float32(np.inf)


# ---------------------------------------------------------------------------------------- the rule
def test_the_rule_on_hand_made_points():
    o = np.zeros((2, 1, 4), bool)                                    # res (4, 1, 2) over [-1, 1]^3: cells of 0.5 in x, 1.0 in z
    o[0, 0, 1] = o[1, 0, 3] = True
    grid = SC.grid_entry(o, [-1, -1, -1], [1, 1, 1])
    xyz = np.array([[[-0.5, 0.0, -0.5],                              # on the low x face of cell (1, 0, 0): in it -> listed
                     [np.nextafter(np.float32(-0.5), np.float32(-1)), 0.0, -0.5],   # just below the face: cell (0, 0, 0) -> skipped
                     [7.0, -9.0, 1e30],                              # outside: clamped to cell (3, 0, 1) -> listed
                     [-7.0, 0.0, -3.0],                              # clamped to cell (0, 0, 0) -> skipped
                     [np.nan, 0.0, 0.0],                             # a NaN coordinate -> listed
                     [0.75, 0.0, 0.0]]], np.float32)                 # z = 0 is the low face of the upper z cell: (3, 0, 1) -> listed
    words, listed = BG.np_background_rows(xyz, grid)
    assert listed.tolist() == [[True, False, True, False, True, True]] and words.tolist() == [0, 2, 4, 5]
    t = np.array([[1.0, 2.0, 3.0, 4.0, np.nan, 6.0]], np.float32)
    for stop, want in ((INF, [0, 2, 4, 5]), (np.float32(3.0), [0, 2, 4]), (np.float32(0.5), [4]), (np.float32(6.0), [0, 2, 4, 5])):
        words, _ = BG.np_background_rows(xyz, grid, t, np.array([stop], np.float32))    # a tie t == t_stop is listed, a NaN depth too
        assert words.tolist() == want, (stop, words)
    # every ray is tested, whatever else the scene does with it: two rays, the second a copy shifted into the empty cells
    two = np.concatenate([xyz, xyz + np.float32([0.5, 0, 0])], 0)
    words, listed = BG.np_background_rows(two, grid)
    assert listed.shape == (2, 6) and (words >> 8).max() == 1


# ---------------------------------------------------------------------------------------- the OccupancyGrids API
def test_flags_defaults_and_refusals():
    g = occ.OccupancyGrids()
    assert g.background is False and g.background_res is None and not g.has_background()
    assert g.background_identity() is None and g.stats()["background"] == (0, 0)
    assert occ.OccupancyGrids(background=True).has_background()
    assert occ.OccupancyGrids(background=True, background_res=(32, 16, 8)).background_res == (32, 16, 8)
    with pytest.raises(TypeError):
        occ.OccupancyGrids(background=1)
    with pytest.raises(ValueError):
        occ.OccupancyGrids(background_res=257)
    ones = torch.ones(2, 2, 2, dtype=torch.bool)
    for layer in (0, -1, False):
        with pytest.raises(ValueError, match="layer 0|cannot carry"):
            g.set_manual(layer, ones, [-1, -1, -1], [1, 1, 1])        # the ray cull's rule stands
    with pytest.raises(ValueError):
        g.set_background_manual(ones)                                # no bounds
    with pytest.raises(ValueError):
        g.set_background_manual(ones.float(), [-1, -1, -1], [1, 1, 1])
    with pytest.raises(ValueError):
        g.set_background_manual(ones, [1, 1, 1], [1, 2, 2])           # lo < hi on every axis
    g.set_background_manual(ones, [-1, -1, -1], [1, 1, 1])
    assert g.has_background() and g.manual_layers() == [] and g.background_identity()[1] == "manual"
    g.set_background_manual(None)
    assert not g.has_background()


def test_the_key_of_a_built_grid_holds_the_frame_id_only_under_the_time_flags():
    lo, hi = np.float32([-3, -3, -3]), np.float32([3, 3, 3])
    g = occ.OccupancyGrids(background=True)
    plain, timed = make_model(), make_model(bkgd_space_time=True)
    assert not g.background_timed(plain) and g.background_timed(timed)
    assert g.background_key(plain, 1.0, lo, hi) == g.background_key(plain, 2.5, lo, hi)          # the frame id is absent
    assert g.background_key(plain, 1.0, lo, hi)[1] is None
    assert g.background_key(timed, 1.0, lo, hi) != g.background_key(timed, 2.5, lo, hi)          # ... and present
    assert g.background_key(timed, 2.5, lo, hi)[1] == 2.5
    timed.use_space_time = False                                      # BKGD_USE_SPACE_TIME acts only under USE_SPACE_TIME
    assert not g.background_timed(timed)
    base = g.background_key(plain, 1.0, lo, hi)
    assert g.background_key(plain, 1.0, lo, hi + np.float32(1e-6)) != base
    assert occ.OccupancyGrids(background=True, background_res=32).background_key(plain, 1.0, lo, hi) != base
    assert occ.OccupancyGrids(background=True, res=32).background_key(plain, 1.0, lo, hi) != base  # background_res None means res
    assert occ.OccupancyGrids(background=True, res=32).background_key(plain, 1.0, lo, hi) == \
        occ.OccupancyGrids(background=True, background_res=32).background_key(plain, 1.0, lo, hi)
    assert occ.OccupancyGrids(background=True, threshold=0.5).background_key(plain, 1.0, lo, hi) != base
    assert occ.OccupancyGrids(background=True, dilate=1).background_key(plain, 1.0, lo, hi) != base
    with torch.no_grad():
        plain.bkgd_spacenet_fine.parameters().__next__().add_(1.0)    # a new parameter version of a background network
    assert g.background_key(plain, 1.0, lo, hi) != base
    performer = g.key(plain, 1, 1.0, lo, hi)
    assert performer != base and base[0] == "bkgd"                    # no clash with a performer's key in the one store


def test_the_fingerprint_keeps_its_length_and_covers_the_background():
    a = occ.OccupancyGrids()
    variants = [occ.OccupancyGrids(background=True), occ.OccupancyGrids(background=True, background_res=32),
                occ.OccupancyGrids(background_res=(32, 16, 8)), occ.OccupancyGrids(samples=True, background=True)]
    prints = [a.fingerprint()] + [v.fingerprint() for v in variants]
    assert all(len(p) == 8 for p in prints) and len({tuple(p) for p in prints}) == len(prints)
    assert all(float(x) == x and abs(x) < 2 ** 53 for p in prints for x in p)
    m = occ.OccupancyGrids()
    m.set_background_manual(torch.ones(2, 2, 2, dtype=torch.bool), [-1, -1, -1], [1, 1, 1])
    m2 = occ.OccupancyGrids()
    m2.set_background_manual(torch.ones(2, 2, 2, dtype=torch.bool), [-1, -1, -1], [1, 1, 2])
    assert len(m.fingerprint()) == 8 and m.fingerprint() != a.fingerprint() and m.fingerprint() != m2.fingerprint()
    m.set_background_manual(None)
    assert m.fingerprint() == a.fingerprint()
    from stnerf_amd.parallel import layers_fingerprint
    model = make_model()
    off = layers_fingerprint(model)
    model.set_occupancy(occ.OccupancyGrids())
    on = layers_fingerprint(model)
    model.set_occupancy(occ.OccupancyGrids(background=True))
    bg = layers_fingerprint(model)
    assert len(off) == len(on) == len(bg) and off != on != bg and off != bg


def test_the_cache_key_is_unchanged_without_a_background_grid_and_changes_with_one():
    model = make_model()
    base = key_of(model)
    model.set_occupancy(occ.OccupancyGrids())                         # performer grids alone: byte-identical key
    assert key_of(model) == base
    model.set_occupancy(occ.OccupancyGrids(samples=True))
    assert key_of(model) == base
    model.set_occupancy(occ.OccupancyGrids(background=True))
    built = key_of(model)
    assert built != base and built[0][:len(base[0])] == base[0] and built[1] == base[1]
    for kw in (dict(background_res=32), dict(res=32), dict(threshold=0.5), dict(dilate=2)):
        model.set_occupancy(occ.OccupancyGrids(background=True, **kw))
        assert key_of(model) not in (base, built), kw
    g = occ.OccupancyGrids()
    model.set_occupancy(g)
    g.set_background_manual(torch.ones(2, 2, 2, dtype=torch.bool), [-3, -3, -3], [3, 3, 3])
    manual = key_of(model)
    assert manual not in (base, built)
    o = torch.ones(2, 2, 2, dtype=torch.bool)
    o[0, 0, 0] = False
    g.set_background_manual(o, [-3, -3, -3], [3, 3, 3])               # a changed grid misses
    assert key_of(model) not in (base, built, manual)
    g.set_background_manual(None)
    assert key_of(model) == base
    model.set_occupancy(None)
    assert key_of(model) == base


def test_the_renderer_switch():
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer

    class Stand:                                                      # (the property alone, on a model without a dataset)
        occupancy = LayeredNeuralRenderer.occupancy

        def __init__(self):
            self.model = make_model()
    r = Stand()
    r.occupancy = "background"
    assert r.occupancy.background and not r.occupancy.samples
    r.occupancy = "samples+background"
    assert r.occupancy.background and r.occupancy.samples
    r.occupancy = "samples"
    assert r.occupancy.samples
    with pytest.raises(TypeError, match="background"):
        r.occupancy = "bkgd"
    r.occupancy = False
    assert r.occupancy is None


def test_the_op_by_op_path_refuses_a_background_grid():
    model = make_model()
    model.set_occupancy(occ.OccupancyGrids(background=True))
    assert "occupancy" in model._inference_only_edits()


# ---------------------------------------------------------------------------------------- argument checks before any launch
def test_the_entries_check_their_arguments_on_the_host():
    lib = hip.lib()
    fake = 1 << 20                                                    # (16-byte aligned, never dereferenced)
    null = C.c_void_p(0)

    def grid(bits=fake, res=(4, 4, 4), lo=(0.0, 0.0, 0.0), inv=(1.0, 1.0, 1.0)):
        g = (hip.Occupancy * 1)()
        g[0].bits = bits
        for a in range(3):
            g[0].res[a], g[0].lo[a], g[0].inv_cell[a] = res[a], lo[a], inv[a]
        return g

    def rows(n=4, ns=8, g=None, t=null, t_stop=null, raw=fake, raw_stride=32, cap=None, counts=null, xyz=fake, rl=fake, rc=fake):
        return lib.stnerf_background_rows(n, xyz, 24, ns, grid() if g is None else g, t, 8, t_stop, raw, raw_stride, rl,
                                          n * ns if cap is None else cap, rc, counts, null)
    bad = [dict(ns=0), dict(ns=257), dict(n=(1 << 23) + 1, ns=1), dict(n=-1), dict(cap=31), dict(g=grid(bits=0)), dict(g=grid(res=(4, 0, 4))),
           dict(g=grid(res=(257, 4, 4))), dict(g=grid(inv=(1.0, float("nan"), 1.0))), dict(g=grid(inv=(1.0, 0.0, 1.0))),
           dict(g=grid(lo=(float("inf"), 0.0, 0.0))), dict(g=grid(bits=fake + 2)), dict(t_stop=fake), dict(raw=fake + 4),
           dict(raw_stride=30), dict(counts=fake + 4), dict(xyz=null), dict(rl=null), dict(rc=null)]
    for kw in bad:
        assert rows(**kw) == hip.EINVAL, kw
        assert "background_rows" in hip.last_error(), (kw, hip.last_error())
    assert lib.stnerf_background_rows(4, fake, 24, 8, None, null, 8, null, fake, 32, fake, 32, fake, null, null) == hip.EINVAL
    # the workspace query: nothing without a grid; one row list with one; shared with layer 0's termination
    n, l, n1, n2 = 1000, 3, 64, 64
    flags = lambda *f: (C.c_int32 * l)(*f)
    W = lib.stnerf_render_workspace_bytes_background
    T = lib.stnerf_render_workspace_bytes_terminated
    plain = lib.stnerf_render_workspace_bytes(n, l, n1, n2, 0)
    row_list = (n * (n1 + n2) * 4 + 255) & ~255
    assert W(n, l, n1, n2, 0, None, None, 0) == plain
    assert W(n, l, n1, n2, 0, None, flags(1, 1, 0), 0) == T(n, l, n1, n2, 0, None, flags(1, 1, 0))
    with_grid = W(n, l, n1, n2, 0, None, None, 1)
    assert plain + row_list <= with_grid <= plain + row_list + 1024
    assert W(n, l, n1, n2, 0, None, flags(1, 1, 0), 1) == T(n, l, n1, n2, 0, None, flags(1, 1, 0))      # layer 0's one list is shared
    assert W(n, l, n1, n2, 0, None, flags(0, 1, 0), 1) == T(n, l, n1, n2, 0, None, flags(0, 1, 0)) + row_list
    assert W(n, l, n1, n2, 0, flags(0, 1, 0), None, 1) == lib.stnerf_render_workspace_bytes_samples(n, l, n1, n2, 0, flags(0, 1, 0)) + row_list
    coarse_list = (n * n1 * 4 + 255) & ~255
    assert W(n, l, n1, n2, 1, None, flags(1, 1, 0), 1) - lib.stnerf_render_workspace_bytes(n, l, n1, n2, 1) in range(coarse_list, coarse_list + 1025)
    assert W(-1, l, n1, n2, 0, None, None, 1) == hip.EINVAL


# ---------------------------------------------------------------------------------------- the oracle-compared cases
def oracle_cases():
    """{name: (case, grid)}: the cases tests/test_gpu_background_grid.py holds against the oracle.  The grid is an x-z checkerboard
    of res 4 over ``bkgd_bbox`` ([-3, 3]^3), the first one tried: on the fp32 oracle it leaves out 2 of the 391 rays and gives 389
    rays with both listed and skipped background samples in either stage (41 % of the coarse, 57 % of the fine samples listed)."""
    out = {}
    for name, case in (("plain", OC.plain_case()), ("full edits", S.make_case()), ("only_coarse", OC.plain_case(only_coarse=True, near=4.0))):
        out[name] = (case, BG.checker_grid(case, (4, 4, 4)))
    return out


@pytest.mark.parametrize("name", ["plain", "full edits", "only_coarse"])
def test_the_oracle_cases_meet_their_two_conditions(monkeypatch, name):
    case, grid = oracle_cases()[name]
    rays = S.case_rays(case)
    ref, stages = BG.oracle_render_background(case, grid, rays, torch.float32, monkeypatch)
    excluded, counts = BG.assert_conditions(case, stages, grid, name)
    print(f"{name}: {int(excluded.sum())} of {rays.shape[0]} rays left out; rays with listed and skipped background samples per stage {counts}")
    assert int(excluded.sum()) <= 2 and min(counts.values()) >= 380, (name, int(excluded.sum()), counts)     # (the figures of the docstring)
    # the wrapped oracle differs from the plain one, and exactly where the rule says: a ray whose background is all listed keeps its bits
    plain = S.oracle_render(case, rays)
    assert S.rays_changed(ref["coarse_layer0"], plain["coarse_layer0"]) >= 100
    final = case["n1"] if case["only_coarse"] else case["n1"] + case["n2"]
    whole = np.ones(rays.shape[0], bool)
    for ns, (_, listed) in stages.items():
        whole &= listed.all(-1)
    for k in ("coarse_layer0", "fine_layer0"):
        assert torch.equal(ref[k][torch.from_numpy(whole)], plain[k][torch.from_numpy(whole)]), (name, k, final)
