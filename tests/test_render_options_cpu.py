"""stnerf_render_options and the ``_opts`` pair (include/stnerf.h), CPU only -- no kernel is launched: the record's size field is
checked before anything else, and the one size query returns what each of the four named queries returns."""
import ctypes as C
import itertools

import pytest

from stnerf_amd import hip

# the shapes test_termination_cpu.py, test_sample_cull_cpu.py and test_background_grid_cpu.py size the workspace for
SHAPES = [(128, 4, 12, 6), (64, 4, 64, 64), (7, 1, 5, 3), (1000, 3, 64, 64)]
# ... and their flag tables (cut or zero-padded to l entries); None: no table
SAMPLES = [None, (0, 0, 0, 0), (0, 1), (0, 1, 0, 1), (0, 1, 1)]
TERMINATE = [None, (0, 0, 0, 0), (1,), (1, 1), (0, 1), (1, 1, 0), (0, 1, 0)]


def _flags(values, l):
    return None if values is None else (C.c_int32 * l)(*(list(values) + [0] * l)[:l])


def _grid():
    """A background grid entry the size query takes as "with bits" (the words are never read on the host)."""
    g = (hip.Occupancy * 1)()
    g[0].bits = C.addressof(g)
    return g


def _render_args(opts):
    """A call that passes the null-pointer check and would fail the next ones: nothing is dereferenced before the size check."""
    null = C.c_void_p(0)
    return (null, 4, null, 0, None, None, null, null, null, 0, null, null, null, null, null, opts, null)


@pytest.mark.parametrize("size", [0, C.sizeof(hip.RenderOptions) + 8])
def test_an_unknown_struct_size_is_refused_before_anything_else(size):
    lib = hip.lib()
    opts = hip.RenderOptions()
    assert opts.struct_size == C.sizeof(hip.RenderOptions)
    opts.struct_size = size
    assert lib.stnerf_render_workspace_bytes_opts(128, 4, 12, 6, 0, C.byref(opts)) == hip.EINVAL
    assert "struct_size" in hip.last_error() and str(size) in hip.last_error()
    # (a bad shape too: the size of the record is looked at first)
    assert lib.stnerf_render_workspace_bytes_opts(-1, 99, 0, 0, 0, C.byref(opts)) == hip.EINVAL and "struct_size" in hip.last_error()
    # the render call: every pointer null, which the call refuses next -- with a good record that is the message
    assert lib.stnerf_render_rays_opts(*_render_args(C.byref(opts))) == hip.EINVAL
    assert "struct_size" in hip.last_error() and str(size) in hip.last_error()
    assert lib.stnerf_render_rays_opts(*_render_args(C.byref(hip.RenderOptions()))) == hip.EINVAL and "null pointer" in hip.last_error()
    assert lib.stnerf_render_rays_opts(*_render_args(None)) == hip.EINVAL and "null pointer" in hip.last_error()


@pytest.mark.parametrize("n,l,n1,n2", SHAPES)
def test_a_null_record_and_a_zeroed_record_give_the_plain_size(n, l, n1, n2):
    lib = hip.lib()
    for only_coarse in (0, 1):
        plain = lib.stnerf_render_workspace_bytes(n, l, n1, n2, only_coarse)
        assert plain > 0
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, None) == plain
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, C.byref(hip.RenderOptions())) == plain
        # what the size does not depend on: every field but samples, terminate and bkgd_grid
        opts = hip.RenderOptions(tau=0.5, occluder_stops=1, scene_out=1 << 20, counts=1 << 20, occluder=1 << 20)
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, C.byref(opts)) == plain
        grid_without_bits = (hip.Occupancy * 1)()
        opts = hip.RenderOptions()
        opts.bkgd_grid = grid_without_bits
        assert lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, C.byref(opts)) == plain
    assert lib.stnerf_render_workspace_bytes_opts(n, 99, n1, n2, 0, None) == hip.EINVAL and "bad shape" in hip.last_error()


@pytest.mark.parametrize("n,l,n1,n2", SHAPES)
def test_the_one_size_query_returns_what_each_named_query_returns(n, l, n1, n2):
    lib = hip.lib()
    grid = _grid()
    checked = 0
    for only_coarse, samples, terminate, background in itertools.product((0, 1), SAMPLES, TERMINATE, (0, 1)):
        sam, ter = _flags(samples, l), _flags(terminate, l)
        opts = hip.RenderOptions()
        opts.samples, opts.terminate = sam, ter
        if background:
            opts.bkgd_grid = grid
        got = lib.stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, C.byref(opts))
        assert got == lib.stnerf_render_workspace_bytes_background(n, l, n1, n2, only_coarse, sam, ter, background), (only_coarse, samples, terminate, background)
        if not background:
            assert got == lib.stnerf_render_workspace_bytes_terminated(n, l, n1, n2, only_coarse, sam, ter)
            if terminate is None:
                assert got == lib.stnerf_render_workspace_bytes_samples(n, l, n1, n2, only_coarse, sam)
                if samples is None:
                    assert got == lib.stnerf_render_workspace_bytes(n, l, n1, n2, only_coarse)
        checked += 1
    assert checked == 2 * len(SAMPLES) * len(TERMINATE) * 2
