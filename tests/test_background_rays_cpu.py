"""The per-ray background mask (include/stnerf.h: "Per-ray background mask"; stnerf_render_options.bkgd_rays;
stnerf_background_ray_rows) and ``ReprojectSpec(exclusive=)``, CPU only -- no kernel is launched: the numpy restatement of the
listing rule on hand-made inputs, every refusal of the built library before any launch, the workspace query, the spec."""
import ctypes as C
import itertools

import numpy as np
import pytest

import background_rays_common as BR
import sample_cull_common as SC
from stnerf_amd import hip
from stnerf_amd.reproject import ReprojectSpec, as_spec

FAKE = 1 << 20                        # (16-byte aligned, never dereferenced)
NULL = C.c_void_p(0)


# ---------------------------------------------------------------------------------------- the rule
def test_the_rule_on_hand_made_inputs():
    occ = np.zeros((2, 2, 2), bool)                       # [Rz][Ry][Rx] over [-1, 1]^3: only the cell x >= 0, y < 0, z < 0 is occupied
    occ[0, 0, 1] = True
    grid = SC.grid_entry(occ, np.float32([-1, -1, -1]), np.float32([1, 1, 1]))
    inside, outside = [0.5, -0.5, -0.5], [-0.5, 0.5, 0.5]
    xyz = np.float32([[inside, outside, [np.nan, 0, 0]], [inside, inside, inside], [outside, outside, outside], [inside, outside, inside]])
    t = np.float32([[1, 2, 3], [1, 2, 3], [1, 2, 3], [1, np.nan, 3]])
    stop = np.float32([2.0, 1.5, np.inf, 0.0])
    flags = np.uint8([1, 0, 200, 1])
    # the mask alone: whole rays, every sample of an "on" ray
    words, listed = BR.np_background_ray_rows(flags, 3)
    assert listed.tolist() == [[True] * 3, [False] * 3, [True] * 3, [True] * 3]
    assert words.tolist() == [0, 1, 2, 512, 513, 514, 768, 769, 770]
    # ... and the grid (a NaN coordinate is listed), ... and the stop depth (a tie and a NaN depth are listed)
    _, listed = BR.np_background_ray_rows(flags, 3, xyz, grid)
    assert listed.tolist() == [[True, False, True], [False] * 3, [False] * 3, [True, False, True]]
    _, listed = BR.np_background_ray_rows(flags, 3, xyz, grid, t, stop)
    assert listed.tolist() == [[True, False, False], [False] * 3, [False] * 3, [False, False, False]]
    _, listed = BR.np_background_ray_rows(flags, 3, t=t, t_stop=stop)
    assert listed.tolist() == [[True, True, False], [False] * 3, [True] * 3, [False, True, False]]
    # all flags on and a grid: the sibling's rule
    import background_grid_common as BG
    w0, l0 = BG.np_background_rows(xyz, grid, t, stop)
    w1, l1 = BR.np_background_ray_rows(np.ones(4, np.uint8), 3, xyz, grid, t, stop)
    assert np.array_equal(w0, w1) and np.array_equal(l0, l1)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 197])
def test_the_flag_patterns(n):
    for name in BR.FLAG_PATTERNS:
        f = BR.flag_pattern(name, n)
        assert f.dtype == np.uint8 and f.shape == (n,)
    assert BR.flag_pattern("all on", n).all() and not BR.flag_pattern("all off", n).any()
    tail = BR.flag_pattern("off only in the ragged last run", n)
    assert int((tail == 0).sum()) == n % 16 and (n < 16 or tail[:n // 16 * 16].all())
    run = BR.flag_pattern("one whole run off", n)
    assert int((run == 0).sum()) == max(0, min(n, 32) - 16)


# ---------------------------------------------------------------------------------------- refusals, before any launch
def _grid(bits=FAKE, res=(4, 4, 4)):
    g = (hip.Occupancy * 1)()
    g[0].bits = bits
    for a in range(3):
        g[0].res[a], g[0].lo[a], g[0].inv_cell[a] = res[a], 0.0, 1.0
    return g


def test_the_stand_alone_entry_checks_its_arguments_on_the_host():
    lib = hip.lib()

    def rows(n=4, ns=8, g=None, t=NULL, t_stop=NULL, raw=FAKE, raw_stride=32, cap=None, counts=NULL, xyz=FAKE, rl=FAKE, rc=FAKE, flags=FAKE):
        return lib.stnerf_background_ray_rows(n, xyz, 24, ns, g, t, 8, t_stop, raw, raw_stride, rl, n * ns if cap is None else cap, rc, counts,
                                              flags, NULL)
    assert rows(flags=NULL) == hip.EINVAL and "ray_flags is required" in hip.last_error()
    assert rows(flags=NULL, g=_grid()) == hip.EINVAL and "ray_flags is required" in hip.last_error()
    # the sibling's checks, with and without a grid (a grid that is given must be a good one with bits)
    bad = [dict(ns=0), dict(ns=257), dict(n=(1 << 23) + 1, ns=1), dict(n=-1), dict(cap=31), dict(t_stop=FAKE), dict(raw=FAKE + 4),
           dict(raw_stride=30), dict(counts=FAKE + 4), dict(xyz=NULL), dict(rl=NULL), dict(rc=NULL)]
    for kw, g in itertools.product(bad, (None, _grid())):
        assert rows(g=g, **kw) == hip.EINVAL, kw
        assert "background_ray_rows" in hip.last_error(), (kw, hip.last_error())
    for g in (_grid(bits=0), _grid(res=(4, 0, 4)), _grid(res=(257, 4, 4)), _grid(bits=FAKE + 2)):
        assert rows(g=g) == hip.EINVAL and "background_ray_rows" in hip.last_error()


def _render_call(n=4, n1=8, n2=4, precision=0, workspace_bytes=1 << 40, only_coarse=0, **fields):
    nets, rp = hip.Nets(), hip.RenderParams()
    rp.l, rp.n1, rp.n2, rp.ray_stride, rp.precision, rp.only_coarse = 3, n1, n2, 9, precision, only_coarse
    nets.bkgd = nets.bkgd_fine = FAKE
    opts = hip.RenderOptions(**fields)
    rc = hip.lib().stnerf_render_rays_opts(FAKE, n, FAKE, 0, C.byref(nets), C.byref(rp), NULL, NULL, FAKE, workspace_bytes, FAKE, FAKE, FAKE,
                                           FAKE, FAKE, C.byref(opts), NULL)
    return rc, hip.last_error()


def test_the_render_call_refuses_what_the_mask_cannot_serve_before_any_launch():
    lib = hip.lib()
    # (n = 0 passes every check and launches nothing: the control of each refusal below)
    assert _render_call(n=0, bkgd_rays=FAKE)[0] == hip.OK
    rc, msg = _render_call(precision=2, bkgd_rays=FAKE)
    assert rc == hip.EINVAL and "per-ray background mask is not built for precision 2" in msg
    assert _render_call(n=0, precision=2, bkgd_rays=FAKE)[0] == hip.EINVAL and _render_call(n=0, precision=2)[0] == hip.OK
    rc, msg = _render_call(n1=200, n2=57, bkgd_rays=FAKE)
    assert rc == hip.EINVAL and "per-ray background mask packs" in msg and "n1 + n2 <= 256" in msg
    assert _render_call(n=0, n1=200, n2=56, bkgd_rays=FAKE)[0] == hip.OK and _render_call(n=0, n1=200, n2=57)[0] == hip.OK
    rc, msg = _render_call(n=(1 << 23) + 1, bkgd_rays=FAKE)
    assert rc == hip.EINVAL and "per-ray background mask packs" in msg and "2^23" in msg
    for mode in (hip.BKGD_CACHE_CAPTURE, hip.BKGD_CACHE_REUSE):
        cache = hip.BkgdCache(FAKE, FAKE, mode)
        rc, msg = _render_call(bkgd_rays=FAKE, cache=C.pointer(cache))
        assert rc == hip.EINVAL and "per-ray background mask with a background cache in CAPTURE or REUSE" in msg, mode
        assert _render_call(n=0, cache=C.pointer(cache))[0] == hip.OK
    off = hip.BkgdCache(0, 0, hip.BKGD_CACHE_OFF)
    assert _render_call(n=0, bkgd_rays=FAKE, cache=C.pointer(off))[0] == hip.OK
    # a workspace of the plain size is too small: layer 0 gets a row list
    for only_coarse in (0, 1):
        plain = lib.stnerf_render_workspace_bytes(4, 3, 8, 4, only_coarse)
        rc, msg = _render_call(workspace_bytes=plain, only_coarse=only_coarse, bkgd_rays=FAKE)
        assert rc == hip.EINVAL and "workspace of" in msg and str(plain) in msg, only_coarse
    assert _render_call(n=0, workspace_bytes=lib.stnerf_render_workspace_bytes(0, 3, 8, 4, 0))[0] == hip.OK
    rc, msg = _render_call(bkgd_rays=FAKE, bkgd_counts=FAKE + 4)
    assert rc == hip.EINVAL and "8-byte aligned" in msg


# ---------------------------------------------------------------------------------------- the workspace query
SHAPES = [(128, 4, 12, 6), (64, 4, 64, 64), (7, 1, 5, 3), (1000, 3, 64, 64)]
TERMINATE = [None, (1,), (0, 1), (1, 1, 0)]
SAMPLES = [None, (0, 1), (0, 1, 1)]


@pytest.mark.parametrize("n,l,n1,n2", SHAPES)
def test_the_workspace_with_a_mask_is_the_workspace_with_a_background_grid(n, l, n1, n2):
    lib = hip.lib()
    flags = lambda v: None if v is None else (C.c_int32 * l)(*(list(v) + [0] * l)[:l])
    grid = _grid()
    for only_coarse, samples, terminate in itertools.product((0, 1), SAMPLES, TERMINATE):
        def query(**fields):
            opts = hip.RenderOptions(**fields)
            opts.samples, opts.terminate = flags(samples), flags(terminate)
            return lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, C.byref(opts))
        none, with_grid, with_mask, both = query(), query(bkgd_grid=grid), query(bkgd_rays=FAKE), query(bkgd_grid=grid, bkgd_rays=FAKE)
        assert with_mask == with_grid == both, (only_coarse, samples, terminate)
        shared = terminate is not None and terminate[0] and not only_coarse          # termination has given layer 0 its list
        assert (with_mask == none) == bool(shared), (only_coarse, samples, terminate)
        row_list = (n * (n1 if only_coarse else n1 + n2) * 4 + 255) & ~255
        assert with_mask - none in ([0] if shared else range(row_list, row_list + 1025))


def test_a_zeroed_record_gives_the_plain_workspace_and_the_python_query_has_the_keyword():
    from stnerf_amd import ops
    lib = hip.lib()
    names = [f for f, _ in hip.RenderOptions._fields_]
    assert names[-1] == "bkgd_rays" and names[-2] == "occluder_share"       # appended: the named entries take a prefix of the record
    opts = hip.RenderOptions()
    assert not opts.bkgd_rays and opts.struct_size == C.sizeof(hip.RenderOptions)
    for n, l, n1, n2 in SHAPES:
        plain = lib.stnerf_render_workspace_bytes(n, l, n1, n2, 0)
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, 0, C.byref(opts)) == plain
        assert ops.render_workspace_bytes(n, l, n1, n2, False) == plain
        assert ops.render_workspace_bytes(n, l, n1, n2, False, background_rays=True) == ops.render_workspace_bytes(n, l, n1, n2, False, background=True) > plain


# ---------------------------------------------------------------------------------------- the spec
def test_the_reproject_spec_takes_exclusive():
    assert ReprojectSpec().exclusive is False and as_spec(dict(key_every=2)).exclusive is False
    assert repr(ReprojectSpec(3, 0.25, 0.5)) == "ReprojectSpec(key_every=3, rel=0.25, a_min=0.5)"           # unchanged for the default
    assert repr(ReprojectSpec(3, 0.25, 0.5, exclusive=False)) == "ReprojectSpec(key_every=3, rel=0.25, a_min=0.5)"
    spec = as_spec(dict(key_every=3, rel=0.25, a_min=0.5, exclusive=True))
    assert spec.exclusive is True and repr(spec) == "ReprojectSpec(key_every=3, rel=0.25, a_min=0.5, exclusive=True)"
    assert spec.keys_of(4, 8) == ReprojectSpec(3).keys_of(4, 8)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="exclusive"):
            ReprojectSpec(exclusive=bad)


def test_absent_rows_is_the_occluders_rule():
    import torch
    from stnerf_amd.reproject import absent_rows
    nan, inf = float("nan"), float("inf")
    rows = torch.tensor([[0, 0, 0, 1.0, 2.0], [0, 0, 0, 0.0, 2.0], [0, 0, 0, -1.0, 2.0], [0, 0, 0, nan, 2.0], [0, 0, 0, 0.5, nan],
                         [0, 0, 0, 0.5, inf], [0, 0, 0, 0.5, -inf], [0, 0, 0, 1e-30, -3.0], [0, 0, 0, 7.0, 0.0]])
    assert absent_rows(rows).tolist() == [False, True, True, True, True, True, True, False, False]
