"""The background cache's host side (no GPU): the key of a launch piece (LayeredRFRender.background_cache_key) holds exactly the
inputs of the background's raw network outputs; stnerf_render_rays_cached / stnerf_copy_layer_raw check their arguments before
any launch; the new symbols are exported and the ctypes mirror of stnerf_bkgd_cache agrees with the header; BackgroundCache's
bookkeeping (budget, statistics, eviction of other groups); the seed is pinned while a cache is attached."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest
import torch

import stnerf_amd
from conftest import REPO
from stnerf_amd import hip, synthetic as syn
from stnerf_amd.bkgd_cache import BackgroundCache, piece_bytes, view_key


def make_model(L=2, bkgd_space_time=False):
    """A model on the HOST: the key is host arithmetic and never touches the weights' values."""
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=bkgd_space_time,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    model = build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=L)), camera_num=1)
    bk, per = syn.scene_boxes(L)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.seed = 11
    model.scale, model.shift = [1.0, 1.0, 1.0], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    return model.eval()


def key_of(model, K=None, T=None, h=17, w=23, frame_ids=(1.0, 1.0, 1.0), piece=(0, 128), window=(0, 0, 0), retiming=True,
           only_coarse=False):
    K0, T0 = syn.camera(17, 23, 15.0)
    return model.background_cache_key(view_key(K0 if K is None else K, T0 if T is None else T, h, w, list(frame_ids)), piece, window,
                                      retiming, only_coarse)


def test_key_ignores_what_does_not_reach_the_background_networks():
    model = make_model()
    base = key_of(model)
    assert base == key_of(model) and hash(base) == hash(key_of(model))
    assert key_of(model, frame_ids=(1.0, 2.5, 3.0)) == base                       # performer frame ids
    assert key_of(model, frame_ids=(2.0, 2.5, 3.0)) == base                       # the background's too: its networks take no time here
    model.hide_layer(1)
    assert key_of(model) == base
    model.show_layer(1)
    model.shift = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.05], [0.0, 0.0, 0.0]]            # performer shift / scale
    model.scale = [1.0, 1.0, 1.2]
    assert key_of(model) == base
    model.alpha = 0.5
    assert key_of(model) == base
    model.set_bboxes(model.bboxes + torch.tensor([0.0, 0.0, 0.0]))                # (a new tensor with the same frame-0 boxes: the pivot stays)
    assert key_of(model) == base
    # the density thresholds are arguments of the render call, not of the key


def test_key_changes_with_every_input_of_the_background_networks():
    model = make_model()
    base = key_of(model)
    K, T = syn.camera(17, 23, 15.0)
    seen = {base}

    def differs(key, what):
        assert key not in seen, what
        seen.add(key)

    differs(key_of(model, T=syn.camera(17, 23, 16.0)[1]), "pose")
    K2 = K.clone()
    K2[0, 0] *= 1.01
    differs(key_of(model, K=K2), "K")
    differs(key_of(model, h=16), "h")
    differs(key_of(model, w=22), "w")
    differs(key_of(model, piece=(128, 256), window=(128, 0, 0)), "piece")
    differs(key_of(model, window=(23, 23, 69)), "ray window")
    assert key_of(model, window=(23, 23, 69))[0] == base[0], "the window belongs to the piece part"
    differs(key_of(model, retiming=False), "ray format")
    differs(key_of(model, only_coarse=True), "only_coarse")
    for attr, value, what in (("seed", 12, "seed"), ("near", 0.5, "near"), ("boarder_weight", 1e9, "border"),
                              ("coarse_ray_sample", 8, "n1"), ("fine_ray_sample", 0, "n2")):
        old = getattr(model, attr)
        setattr(model, attr, value)
        differs(key_of(model), what)
        setattr(model, attr, old)
        assert key_of(model) == base, what
    model.shift = [[0.1, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    differs(key_of(model), "layer-0 shift")
    model.shift = [None, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]                        # (fine: no un-edit at all for layer 0)
    differs(key_of(model), "layer-0 shift None")
    model.shift = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]
    model.scale = [1.1, 1.0, 1.0]
    differs(key_of(model), "layer-0 scale")
    model.scale = None
    differs(key_of(model), "no scale edit (no pivot, no scale-1 un-edit of layer 0)")
    model.scale = [1.0, 1.0, 1.0]
    assert key_of(model) == base
    bk = model.bkgd_bbox
    model.set_bkgd_bbox(bk * 0.9)
    differs(key_of(model), "background box")
    model.set_bkgd_bbox(bk)
    assert key_of(model) == base
    bk.mul_(0.5)                                                                   # (in place: the host copy follows the version)
    differs(key_of(model), "background box, in place")
    bk.mul_(2.0)
    model.set_precision("fp32")
    differs(key_of(model), "precision")
    model.mlp_schedule = "per_net"
    differs(key_of(model), "schedule (exact f32)")
    model.set_precision("bf16x3")
    assert key_of(model) == base, "the split-bf16 arithmetic has one schedule"
    model.mlp_schedule = "stage"
    for net, what in ((model.bkgd_spacenet, "bkgd_spacenet"), (model.bkgd_spacenet_fine, "bkgd_spacenet_fine")):
        with torch.no_grad():
            next(net.parameters()).add_(1e-3)
        differs(key_of(model), what + " parameter update")
    fp = key_of(model)
    with torch.no_grad():
        next(model.spacenets[0].parameters()).add_(1e-3)                           # a performer's network: not the background's business
        next(model.time_deform_nets[1].parameters()).add_(1e-3)
    assert key_of(model) == fp
    # the background's frame id is an input of its networks only with BKGD_USE_SPACE_TIME / BKGD_USE_DEFORM_TIME
    timed = make_model(bkgd_space_time=True)
    t1 = key_of(timed, frame_ids=(1.0, 1.0, 1.0))
    assert key_of(timed, frame_ids=(1.0, 2.5, 3.0)) == t1
    assert key_of(timed, frame_ids=(2.0, 1.0, 1.0)) != t1
    assert t1 != base                                                              # (other flags, other networks)


def test_key_without_performers_and_without_edits():
    model = make_model(L=0)
    model.scale = model.shift = None
    k = key_of(model, frame_ids=(1.0,), retiming=False)
    assert k == key_of(model, frame_ids=(2.0,), retiming=False)
    model.near = 1.0
    assert k != key_of(model, frame_ids=(1.0,), retiming=False)


@pytest.fixture(scope="module")
def lib():
    return hip.lib()


def test_new_symbols_are_exported(lib):
    for name in ("stnerf_render_rays_cached", "stnerf_copy_layer_raw"):
        assert name in hip.exported_symbols() and getattr(lib, name) is not None
    header = open(os.path.join(REPO, "include", "stnerf.h")).read()
    assert "stnerf_render_rays_cached(" in header and "stnerf_copy_layer_raw(" in header
    assert stnerf_amd.BackgroundCache is BackgroundCache
    from stnerf_amd import ops
    assert ops.PROFILE_KERNELS[6] == "copy_layer_raw"


def test_cache_struct_matches_the_header(tmp_path):
    assert C.sizeof(hip.BkgdCache) == 24
    assert [getattr(hip.BkgdCache, f).offset for f, _ in hip.BkgdCache._fields_] == [0, 8, 16]
    assert (hip.BKGD_CACHE_OFF, hip.BKGD_CACHE_CAPTURE, hip.BKGD_CACHE_REUSE) == (0, 1, 2)
    gcc = shutil.which("gcc")
    if gcc is None:
        return                                   # (the constants above are the x86-64 / LP64 layout of the header's struct)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stnerf.h"', 'int main(void){',
             'printf("%zu\\n", sizeof(stnerf_bkgd_cache));']
    lines += [f'printf("%zu\\n", offsetof(stnerf_bkgd_cache, {f}));' for f, _ in hip.BkgdCache._fields_]
    lines += ['printf("%d %d %d\\n", STNERF_BKGD_CACHE_OFF, STNERF_BKGD_CACHE_CAPTURE, STNERF_BKGD_CACHE_REUSE);', 'return 0;}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [24, 0, 8, 16, 0, 1, 2]


def test_cached_entry_checks_its_arguments_before_any_launch(lib):
    fake = 1 << 20                                # (16-byte aligned, never dereferenced)
    null = C.c_void_p(0)
    nets = hip.Nets()
    nets.bkgd = nets.bkgd_fine = fake
    p = hip.RenderParams()
    p.l, p.n1, p.n2, p.ray_stride, p.precision = 1, 12, 6, 7, 3

    def call(cache, n=4, only_coarse=0):
        p.only_coarse = only_coarse
        return lib.stnerf_render_rays_cached(fake, n, fake, 0, C.byref(nets), C.byref(p), null, null, fake, 1 << 30, fake, fake, fake, fake,
                                             fake, None if cache is None else C.byref(cache), None)

    assert call(hip.BkgdCache(fake, fake, 7)) == hip.EINVAL and "cache mode 7" in hip.last_error()
    assert call(hip.BkgdCache(fake, fake, -1)) == hip.EINVAL
    for mode in (hip.BKGD_CACHE_CAPTURE, hip.BKGD_CACHE_REUSE):
        assert call(hip.BkgdCache(None, fake, mode)) == hip.EINVAL and "raw_coarse" in hip.last_error()
        assert call(hip.BkgdCache(fake, None, mode)) == hip.EINVAL and "raw_fine" in hip.last_error()
        assert call(hip.BkgdCache(fake + 4, fake, mode)) == hip.EINVAL and "16-byte aligned" in hip.last_error()
        assert call(hip.BkgdCache(fake, fake + 8, mode)) == hip.EINVAL and "16-byte aligned" in hip.last_error()
        assert call(hip.BkgdCache(None, None, mode), only_coarse=1) == hip.EINVAL
        # a well-formed cache passes the checks (n = 0: nothing to launch); raw_fine is not needed with only_coarse
        assert call(hip.BkgdCache(fake, fake, mode), n=0) == hip.OK
        assert call(hip.BkgdCache(fake, None, mode), n=0, only_coarse=1) == hip.OK
        assert call(hip.BkgdCache(fake, fake + 8, mode), n=0, only_coarse=1) == hip.OK
    assert call(hip.BkgdCache(None, None, hip.BKGD_CACHE_OFF), n=0) == hip.OK     # mode 0: the buffers are not looked at
    assert call(None, n=0) == hip.OK
    # the other arguments are checked as in stnerf_render_rays
    assert lib.stnerf_render_rays_cached(null, 4, null, 0, None, None, null, null, null, 0, null, null, null, null, null, None, None) == hip.EINVAL

    copy = lambda raw, n, l, layer, ns, dense, to_dense=1: lib.stnerf_copy_layer_raw(raw, n, l, layer, ns, dense, to_dense, None)
    assert copy(null, 4, 3, 0, 8, fake) == hip.EINVAL and "null pointer" in hip.last_error()
    assert copy(fake, 4, 3, 0, 8, null) == hip.EINVAL
    assert copy(fake, 4, 3, 3, 8, fake) == hip.EINVAL and "bad shape" in hip.last_error()
    assert copy(fake, 4, 3, -1, 8, fake) == hip.EINVAL
    assert copy(fake, 4, 0, 0, 8, fake) == hip.EINVAL
    assert copy(fake, 4, 17, 0, 8, fake) == hip.EINVAL
    assert copy(fake, 4, 3, 0, 0, fake) == hip.EINVAL
    assert copy(fake, -1, 3, 0, 8, fake) == hip.EINVAL
    assert copy(fake + 4, 4, 3, 0, 8, fake) == hip.EINVAL and "16-byte aligned" in hip.last_error()
    assert copy(fake, 4, 3, 0, 8, fake + 8, 0) == hip.EINVAL
    assert copy(fake, 0, 3, 0, 8, fake) == hip.OK                                  # nothing to copy: no launch


def test_cache_bookkeeping_budget_and_eviction(monkeypatch):
    one = piece_bytes(128, 12, 6, False)
    assert one == 16 * 128 * 30 and piece_bytes(128, 12, 6, True) == 16 * 128 * 12
    assert piece_bytes(1920 * 1080, 64, 64, False) == 3072 * 1920 * 1080            # 3 KB per ray at 64 + 64: 6.4 GB for a 1080p view
    cache = BackgroundCache(max_bytes=2 * one)
    a, b, c = ("A", (0, 128, (0, 0, 0))), ("A", (128, 256, (128, 0, 0))), ("A", (256, 384, (256, 0, 0)))
    assert cache.lookup(a) is None
    raw_c, raw_f = cache.reserve(a, 128, 12, 6, False, "cpu")
    assert tuple(raw_c.shape) == (128, 12, 4) and tuple(raw_f.shape) == (128, 18, 4) and raw_c.dtype == torch.float32
    assert cache.lookup(a)[0] is raw_c
    assert cache.reserve(b, 128, 12, 6, False, "cpu") is not None
    assert cache.reserve(c, 128, 12, 6, False, "cpu") is None                       # the same group's pieces are not evicted for it
    assert cache.stats == dict(hits=1, misses=1, captures=2, skipped_over_budget=1) and cache.bytes_used == 2 * one and len(cache) == 2
    other = ("B", (0, 128, (0, 0, 0)))
    assert cache.reserve(other, 128, 12, 6, False, "cpu") is not None               # another group (view, seed, weights ...): oldest out
    assert cache.lookup(a) is None and cache.lookup(b) is not None and cache.bytes_used == 2 * one
    assert cache.reserve(("B", (0, 64, (0, 0, 0))), 64, 12, 6, True, "cpu")[1] is None   # only_coarse: no fine slice; evicts group A's last
    assert cache.lookup(b) is None and cache.bytes_used == one + piece_bytes(64, 12, 6, True)
    cache.clear()
    assert len(cache) == 0 and cache.bytes_used == 0 and cache.stats["captures"] == 4
    assert BackgroundCache().max_bytes == 8 << 30
    monkeypatch.setenv("STNERF_BKGD_CACHE_GB", "0.5")
    assert BackgroundCache().max_bytes == 1 << 29 and BackgroundCache(max_bytes=7).max_bytes == 7


def test_view_tag_follows_the_tensor_only():
    from stnerf_amd.bkgd_cache import tag_view_rays, tagged_view_key
    K, T = syn.camera(17, 23, 15.0)
    rays = torch.zeros(17 * 23, 9)
    assert tagged_view_key(rays) is None
    assert tag_view_rays(rays, K, T, 17, 23, [1.0, 2.5, 3.0]) is rays
    assert tagged_view_key(rays) == view_key(K, T, 17, 23, [1.0, 2.5, 3.0]) and tagged_view_key(rays)[1] == 1.0
    assert tagged_view_key(rays.to("cpu")) is not None                 # (the same tensor)
    assert tagged_view_key(rays.clone()) is None and tagged_view_key(rays[:64]) is None
    rays[0, 0] = 1.0                                                   # written to since: the tag no longer vouches for it
    assert tagged_view_key(rays) is None


def test_seed_is_pinned_and_the_renderer_switch_attaches():
    model = make_model()
    model.fresh_draws_per_call = True
    model.advance_seed()
    assert model.seed == 12
    assert model.set_background_cache(BackgroundCache()) is model
    model.advance_seed()
    assert model.seed == 12
    model.set_background_cache(None)
    model.advance_seed()
    assert model.seed == 13
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[23, 17]))
    K, T = syn.camera(17, 23, 15.0)
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K])
    assert r.cache_background is False and model._bkgd_cache is None
    r.cache_background = True
    held = model._bkgd_cache
    assert r.cache_background is True and isinstance(held, BackgroundCache)
    r.cache_background = True
    assert model._bkgd_cache is held                                                 # (already on: the cache is kept)
    r.cache_background = False
    assert model._bkgd_cache is None
    assert LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], cache_background=True).cache_background is True
    with pytest.raises(TypeError):
        LayeredNeuralRenderer(cfg, None, None, None, None, None, None, True)         # keyword-only: the positional signature is the reference's
