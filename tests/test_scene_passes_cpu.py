"""In-scene layer passes, host side (no GPU): the header declares the new entries and leaves the old structs alone, the library
exports them and checks their arguments before anything is launched, the production compositor kernels keep their registers
beside the new instantiations, the ops refuse CPU tensors, and the renderer's ``scene_passes`` bookkeeping against a stub model."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import tools.asm_listing as asm
from conftest import REPO
from stnerf_amd import hip, ops, synthetic as syn

HEADER = open(os.path.join(REPO, "include", "stnerf.h")).read()
NEW = ("stnerf_composite_scene", "stnerf_render_rays_scene")


def test_header_declares_the_new_entries():
    for name in NEW:
        assert len(re.findall(r"^int " + name + r"\(", HEADER, re.M)) == 1, name
        assert name in hip.exported_symbols()
    decl = HEADER[HEADER.index("int stnerf_composite_scene("):]
    decl = decl[:decl.index(";")]
    assert "float* merged_weights, float* scene_out" in decl
    decl = HEADER[HEADER.index("int stnerf_render_rays_scene("):]
    decl = decl[:decl.index(";")]
    assert "float* scene_out" in decl and "rotations_host" in decl and "cache_host" in decl
    # the old entries are still declared, with the argument lists they had
    old = HEADER[HEADER.index("int stnerf_composite("):]
    assert old[:old.index(";")].count(",") == 12
    old = HEADER[HEADER.index("int stnerf_render_rays_rot("):]
    assert old[:old.index(";")].count(",") == 17


def test_struct_sizes_of_the_old_entries_are_unchanged(tmp_path):
    sizes = {"stnerf_composite_params": (hip.CompositeParams, 276), "stnerf_render_params": (hip.RenderParams, 952),
             "stnerf_nets": (hip.Nets, 400), "stnerf_bkgd_cache": (hip.BkgdCache, 24), "stnerf_layer_rotation": (hip.LayerRotation, 52),
             "stnerf_layer_edit": (hip.LayerEdit, 24)}
    for cname, (cls, size) in sizes.items():
        assert C.sizeof(cls) == size, (cname, C.sizeof(cls))
    gcc = shutil.which("gcc")
    if gcc is None:
        return                                   # (the constants above are the x86-64 / LP64 layout of the header's structs)
    lines = ['#include <stdio.h>', '#include "stnerf.h"', 'int main(void){']
    lines += [f'printf("{cname} %zu\\n", sizeof({cname}));' for cname in sizes]
    lines.append('return 0;}')
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, (cls, size) in sizes.items():
        assert int(got[cname]) == size, cname


def test_library_exports_the_entries_and_checks_arguments_on_the_host():
    lib = hip.lib()
    for name in NEW:
        assert getattr(lib, name) is not None
    null, fake = C.c_void_p(0), 1 << 20
    p = ops.composite_params()
    # scene_out without merged_weights; merged_weights without mixed_out; both before any launch (the pointers are made up)
    assert lib.stnerf_composite_scene(fake, fake, null, 8, 3, 64, C.byref(p), fake, fake, null, null, null, null, fake, null) == hip.EINVAL
    assert "scene_out needs merged_weights" in hip.last_error()
    assert lib.stnerf_composite_scene(fake, fake, null, 8, 3, 64, C.byref(p), fake, null, null, null, null, fake, null, null) == hip.EINVAL
    assert "merged_weights needs mixed_out" in hip.last_error()
    assert lib.stnerf_composite_scene(fake, fake, null, 0, 3, 64, C.byref(p), fake, fake, null, null, null, fake, fake, null) == hip.OK
    assert lib.stnerf_composite_scene(null, null, null, 8, 3, 64, None, null, null, null, null, null, null, null, null) == hip.EINVAL
    assert lib.stnerf_render_rays_scene(null, 4, null, 0, None, None, null, null, null, 0, null, null, null, null, null, None, None, fake,
                                        null) == hip.EINVAL
    # the workspace query is what it was: the merged weights live in the final stage's point buffer
    for (n, l, n1, n2, oc), want in (((1000, 3, 64, 64, 0), None), ((391, 3, 12, 6, 1), None)):
        S = n1 + n2
        pad = lambda f: (f + 63) // 64 * 64
        t_c, xyz_c, raw_c = n * l * n1, n * l * n1 * 3, n * l * n1 * 4
        w_c, slots = (0, 0) if oc else (n * l * n1, n * n2)
        t_f, xyz_f, raw_f = (0, 0, 0) if oc else (n * l * S, n * l * S * 3, n * l * S * 4)
        tail = max(pad(raw_c) + pad(w_c), pad(slots))
        shared = max(pad(t_c) + pad(xyz_c) + tail, pad(raw_f))
        count = 16 + 2 + 32
        assert ops.render_workspace_bytes(n, l, n1, n2, bool(oc)) == (shared + t_f + xyz_f + l * n * 128) * 4 + (l * n + count) * 4 + n + 16 * 256
        assert (xyz_c if oc else xyz_f) >= n * l * (n1 if oc else S)      # room for the alias


def test_ops_refuse_cpu_tensors():
    t, raw = torch.zeros(4, 3, 8), torch.zeros(4, 3, 8, 4)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.composite_scene(t, raw, None)
    nets, params = hip.Nets(), hip.RenderParams()
    params.l, params.n1, params.n2, params.ray_stride = 3, 8, 4, 9
    boxes = torch.zeros(3, 8, 3)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.render_rays(torch.zeros(4, 9), boxes, nets, params, torch.zeros(16, dtype=torch.uint8), scene=True)


@asm.needs_hipcc
def test_compositor_instantiations_resources():
    """The instantiations a render without the pass launches come first in the object and keep their occupancy targets (what
    tests/test_kernel_resources.py reads); the ones that write merged_weights and layer_scene_kernel use no scratch, and the new
    kernel loads its colours as vectors."""
    kernels = asm.kernels(asm.listing("composite.hip"))
    names = [n for n in kernels if re.fullmatch(r"_ZN6stnerf\w+", n)]

    def kernel(name):
        k = kernels[name]
        return k["body"], k["NumVgprs"], k["ScratchSize"], k["Occupancy"]

    merge = [n for n in names if "composite_merge_kernel" in n]
    assert len(merge) == 12 and all("ELb0EEE" in n for n in merge[:6]) and all("ELb1EEE" in n for n in merge[6:]), merge
    target = {("1", "1"): 7, ("2", "1"): 7, ("3", "1"): 6, ("1", "0"): 5, ("2", "0"): 5, ("3", "0"): 5}     # merge_waves_per_simd
    for n in merge:
        maxb, full, mw = re.search(r"ILi(\d)ELb([01])ELb([01])EEE", n).groups()
        _, vgprs, scratch, occ = kernel(n)
        assert scratch == 0, (n, scratch)
        assert occ >= target[maxb, full] - (1 if mw == "1" and full == "1" else 0), (n, vgprs, occ)
    single = [n for n in names if "composite_single_kernel" in n]
    assert len(single) == 4
    for n in single:
        _, vgprs, scratch, occ = kernel(n)
        assert scratch == 0 and occ >= (4 if "ILi3E" in n else 6), (n, vgprs, occ)      # STNERF_WAVES_SINGLE
    scene = [n for n in names if "layer_scene_kernel" in n]
    assert len(scene) == 1
    body, vgprs, scratch, occ = kernel(scene[0])
    assert scratch == 0 and occ == 8, (vgprs, occ)
    # three blocks of colours per round trip, as vectors (the unused density is dropped from the 16-byte load: dwordx3)
    assert len(re.findall(r"global_load_dwordx[34] ", body)) >= 3 and "v_add_f32_dpp" in body


# ---- the renderer's bookkeeping against a stub model
class StubModel:
    layer_num = 2

    def __init__(self):
        self.scale = self.shift = self.rotation = None
        self.calls = []

    def hide_layer(self, i):
        pass

    def show_layer(self, i):
        pass


def make_renderer(scene_passes, monkeypatch):
    from stnerf_amd.render import layered_neural_renderer as lnr
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[6, 4]))
    K, T = syn.camera(4, 6, 15.0)
    model = StubModel()

    def fake_render_pose(model_, pose, K_, h, w, pairs, far, thr=0, bthr=0, device="cuda", scene_passes=False):
        model_.calls.append(scene_passes)
        g = torch.Generator().manual_seed(len(model_.calls))
        color, depth = torch.rand(h, w, 3, generator=g), torch.rand(h, w, 1, generator=g)
        color_layer = [torch.rand(h, w, 3, generator=g) for _ in range(3)]
        color_layer[2][0, 0] = 0.0
        depth_layer = [torch.rand(h, w, 1, generator=g) for _ in range(3)]
        if not scene_passes:
            return color, depth, color_layer, depth_layer
        passes = dict(color_scene=[torch.rand(h, w, 3, generator=g) for _ in range(3)],
                      alpha_scene=[torch.rand(h, w, 1, generator=g) for _ in range(3)],
                      depth_scene=[torch.rand(h, w, 1, generator=g) for _ in range(3)])
        return color, depth, color_layer, depth_layer, passes

    monkeypatch.setattr(lnr, "_render_pose", fake_render_pose)
    kw = dict(scene_passes=True) if scene_passes else {}
    r = lnr.LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], **kw)
    r.set_path_fixed_gt_poses(0, 3)
    return r, model


@pytest.mark.parametrize("walking", [False, True])
def test_renderer_scene_passes_bookkeeping(monkeypatch, walking):
    from stnerf_amd.render.layered_neural_renderer import LayeredNeuralRenderer
    run = lambda r, **kw: (r.render_path_walking if walking else r.render_path)(**kw)
    # flag off: the five-argument callback still works, no pass is asked for, the lists stay empty
    r0, m0 = make_renderer(False, monkeypatch)
    seen0 = []
    run(r0, on_frame=lambda idx, c, d, cl, dl: seen0.append((idx, c, cl)))
    assert len(seen0) == 3 and m0.calls == [False] * 3 and r0.scene_passes is False
    assert all(len(x) == 0 for x in r0.images_scene) and all(len(x) == 0 for x in r0.alphas_scene)
    # flag on: the keyword arrives, the lists fill next to images_layer
    r1, m1 = make_renderer(True, monkeypatch)
    seen1 = []
    run(r1, inverse_y_axis=True, on_frame=lambda idx, c, d, cl, dl, scene=None: seen1.append((idx, c, cl, scene)))
    assert m1.calls == [True] * 3 and len(seen1) == 3
    for idx, c, cl, sc in seen1:
        assert sorted(sc) == ["alpha_scene", "color_scene", "depth_scene"] and all(len(v) == 3 for v in sc.values())
    for layer in range(3):
        assert len(r1.images_scene[layer]) == len(r1.alphas_scene[layer]) == len(r1.images_layer[layer]) == 3
        for k in range(3):
            assert torch.equal(r1.images_scene[layer][k], seen1[k][3]["color_scene"][layer])
            assert torch.equal(r1.alphas_scene[layer][k], seen1[k][3]["alpha_scene"][layer])
            assert r1.images_scene[layer][k].shape == (4, 6, 3) and r1.alphas_scene[layer][k].shape == (4, 6, 1)
    # the stub draws the same standard outputs with the flag on and off: what the renderer keeps of them is unchanged (flipped here)
    for k in range(3):
        assert torch.equal(r1.images[k], torch.flip(r0.images[k], [0]))
        assert torch.equal(r1.images_layer[1][k], torch.flip(r0.images_layer[1][k], [0]))
    if walking:          # color_hide stays the reference's computation (:606-611), on the flag's both settings
        assert len(r0.images_hide) == len(r1.images_hide) == 3
        for k in range(3):
            cl, dl = [x[k] for x in r0.images_layer], [x[k] for x in r0.depths_layer]
            want = cl[0].clone()
            index = dl[2] < dl[0]
            index = torch.logical_and(torch.cat([index, index, index], dim=2), cl[2] != 0)
            want[index] = cl[2][index]
            assert torch.equal(r0.images_hide[k], want) and torch.equal(r1.images_hide[k], torch.flip(want, [0]))
    with pytest.raises(TypeError):
        LayeredNeuralRenderer(r0.cfg, None, None, None, None, None, None, False, None, True)          # keyword-only


def test_render_rays_scene_refuses_training_mode_and_sharded_views(monkeypatch):
    from stnerf_amd import parallel
    from stnerf_amd.modeling import build_layered_model
    m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                              POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                              USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                              DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
    model = build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=2)), camera_num=1)
    rays = torch.zeros(4, 9)
    model.train()
    with pytest.raises(RuntimeError, match="training mode"):
        model.render_rays_scene(rays)
    model.eval()
    monkeypatch.setattr(parallel.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(parallel.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(parallel.dist, "get_rank", lambda group=None: 0)
    model.shard_views = True
    with torch.no_grad(), pytest.raises(RuntimeError, match="scene.*gather mode"):
        model.render_rays_scene(rays)
    with torch.no_grad(), pytest.raises(RuntimeError, match="scene.*gather mode"):
        K, T = syn.camera(64, 64, 15.0)
        parallel.render_view(model, K, T, 64, 64, [1.0, 1.0, 1.0], chuncks=512, device="cpu", scene=True)
    model.shard_views = False
    with torch.no_grad(), pytest.raises(RuntimeError, match="must live on the GPU"):
        model.render_rays_scene(rays)             # (one rank, eval mode: the call goes on to the render path, which has no CPU form)
