"""Per-layer rotation on the GPU (include/stnerf.h: stnerf_layer_rotation).  A rotated layer sees the ray in its own frame and is
then rendered as an unrotated one, so every check is bit for bit against the rotation-free code on ROTATED RAYS: rays' computed
here with torch fp32 operations in the stated order from the (m, c) of ``LayeredRFRender.layer_ray_transforms``, frame-id columns
copied.  Shapes as tests/test_gpu_bkgd_cache.py: views of 23 x 17 = 391 rays (no multiple of 64) in launch pieces of 128 (the last
one of 7 rays), reference chunks of 64, (n1, n2) = (12, 6) and (8, 0), two performers."""
import math
import types

import pytest
import torch

import stnerf_amd
from stnerf_amd import ops, synthetic as syn
from stnerf_amd.bkgd_cache import view_key

pytestmark = pytest.mark.gpu

H, W, CAP, CHUNK = 17, 23, 128, 64
N = H * W
PIECES = (N + CAP - 1) // CAP
CENTRE = (0.1, -0.2, 0.05)


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=torch.float64)


TILTED = rot_z(0.6) @ rot_x(0.35)          # a general rotation: about z, with a tilt

_MODEL = []


def make_model(n1=12, n2=6, precision="bf16x3", schedule="stage"):
    """The two-performer synthetic model in a known state (built and uploaded once)."""
    if not _MODEL:
        from stnerf_amd.modeling import build_layered_model
        m = types.SimpleNamespace(BOARDER_WEIGHT=1e10, SAMPLE_METHOD="BBOX", SAME_SPACENET=False, TKERNEL_INC_RAW=True,
                                  POSE_REFINEMENT=False, USE_DIR=True, USE_DEFORM_VIEW=False, USE_DEFORM_TIME=True,
                                  USE_SPACE_TIME=True, BKGD_USE_DEFORM_TIME=False, BKGD_USE_SPACE_TIME=False,
                                  DEEP_RGB=False, COARSE_RAY_SAMPLING=12, FINE_RAY_SAMPLING=6)
        model = build_layered_model(types.SimpleNamespace(MODEL=m, DATASETS=types.SimpleNamespace(LAYER_NUM=2)), camera_num=1)
        model.load_state_dict(syn.make_state_dict(2, True, True, seed=3))
        _MODEL.append(model.cuda().eval())
    model = _MODEL[0]
    bk, per = syn.scene_boxes(2)
    model.set_bkgd_bbox(bk)
    model.set_bboxes(per)
    model.coarse_ray_sample, model.fine_ray_sample = n1, n2
    model.set_precision(precision)
    model.mlp_schedule = schedule
    model.max_rays_per_launch = CAP
    model.seed, model.fresh_draws_per_call = 11, False
    model.scale = model.shift = model.rotation = None
    model.near, model.alpha = 0, 1
    for i in range(3):
        model.show_layer(i)
    model.set_background_cache(None)
    return model


def rotated_rays(rays, m, c):
    """rays' of the header's formula, one fp32 operation at a time (on the host: ATen's CPU kernels fuse nothing)."""
    r = rays.detach().cpu()
    m, c = m.to(torch.float32), c.to(torch.float32)
    o, d = r[:, 0:3], r[:, 3:6]
    q = [o[:, j] - c[j] for j in range(3)]
    out = r.clone()
    for k in range(3):
        out[:, k] = ((m[k, 0] * q[0] + m[k, 1] * q[1]) + m[k, 2] * q[2]) + c[k]
        out[:, 3 + k] = (m[k, 0] * d[:, 0] + m[k, 1] * d[:, 1]) + m[k, 2] * d[:, 2]
    return out.to(rays.device)


def render(model, rays, only_coarse=False):
    with torch.no_grad():
        out = model.render_rays_raw(rays, only_coarse, 0.0, 0.0, ref_chunk=CHUNK)
    torch.cuda.synchronize()
    return [o.clone() for o in out]


def bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def assert_bit_equal(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    a, b = bits(got), bits(ref)
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ"


def view_rays(retiming=True, orbit=15.0, frames=(1.0, 2.5, 3.0)):
    K, T = syn.camera(H, W, orbit)
    return ops.generate_rays(K, T, H, W, frame_ids=list(frames) if retiming else [2.0])


# ---- 1. the whole scene turned: every layer carries the same rotation about one centre
@pytest.mark.parametrize("precision,schedule,retiming,only_coarse,edits,n1,n2,spec", [
    ("bf16x3", "stage", True, False, False, 12, 6, 0.6),
    ("fp32", "stage", True, False, False, 12, 6, TILTED),
    ("fp32", "per_net", True, False, False, 12, 6, 0.6),
    ("bf16x3", "stage", False, False, False, 12, 6, TILTED),
    ("fp32", "per_net", False, False, False, 12, 6, 0.6),
    ("bf16x3", "stage", True, True, False, 12, 6, 0.6),
    ("fp32", "stage", False, True, False, 12, 6, TILTED),
    ("bf16x3", "stage", True, False, True, 12, 6, TILTED),
    ("bf16x3", "stage", True, False, False, 8, 0, 0.6),
])
def test_whole_scene_rotation_equals_the_plain_render_of_rotated_rays(precision, schedule, retiming, only_coarse, edits, n1, n2, spec):
    model = make_model(n1, n2, precision, schedule)
    if edits:
        model.scale, model.shift = [1.0, 1.2, 0.9], [[0.0, 0.0, 0.0], [0.1, 0.0, 0.05], [-0.05, 0.1, 0.0]]
    rays = view_rays(retiming)
    assert rays.shape == (N, 9 if retiming else 7)
    model.rotation = [(spec, CENTRE)] * 3
    tr = model.layer_ray_transforms(None)
    assert all(torch.equal(tr[i][0], tr[0][0]) and torch.equal(tr[i][1], tr[0][1]) for i in range(3))
    got = render(model, rays, only_coarse)
    model.rotation = None
    turned = rotated_rays(rays, *tr[0])
    assert torch.equal(turned[:, 6:], rays[:, 6:]) and not torch.equal(turned[:, :6], rays[:, :6])
    ref = render(model, turned, only_coarse)
    for k, name in enumerate(("mixed_fine", "mixed_coarse", "layer_fine", "layer_coarse", "mask")):
        assert_bit_equal(got[k], ref[k], name)
    plain = render(model, rays, only_coarse)
    assert not torch.equal(got[1], plain[1]), "the rotation did not change the image"


# ---- 2. one performer turned in place: its layer is the plain one on rotated rays, the others are untouched
@pytest.mark.parametrize("precision,schedule", [("bf16x3", "stage"), ("fp32", "stage"), ("fp32", "per_net")])
def test_one_rotated_layer(precision, schedule):
    model = make_model(12, 6, precision, schedule)
    rays = view_rays(True, orbit=25.0, frames=(1.0, 1.0, 1.0))
    model.rotation = [None, 0.6, None]
    boxes, _ = model._retimed_boxes(rays[0, 6:].cpu())
    tr = model.layer_ray_transforms(boxes)
    assert tr[0] is None and tr[2] is None and torch.equal(tr[1][1], torch.mean(boxes[1], 0))
    got = render(model, rays)
    model.rotation = None
    plain = render(model, rays)
    turned = render(model, rotated_rays(rays, *tr[1]))
    for k, name in ((2, "layer_fine"), (3, "layer_coarse"), (4, "mask")):
        assert_bit_equal(got[k][:, 1], turned[k][:, 1], f"{name} of the rotated layer")
        for i in (0, 2):
            assert_bit_equal(got[k][:, i], plain[k][:, i], f"{name} of layer {i}")
    hit = got[4][:, 1] != 0
    miss_both = (got[4][:, 1] == 0) & (plain[4][:, 1] == 0)
    # (the CPU oracle counts 152 of the 391 rays on the layer at angle 0.6 and 159 unrotated)
    assert int(hit.sum()) >= 0.15 * N and int(miss_both.sum()) >= 0.15 * N, (int(hit.sum()), int(miss_both.sum()))
    for k, name in ((0, "mixed_fine"), (1, "mixed_coarse")):
        assert_bit_equal(got[k][miss_both], plain[k][miss_both], f"{name} on rays that miss the layer in both renders")
        assert bool((bits(got[k][hit]) != bits(plain[k][hit])).any()), f"{name}: no ray that hits the rotated layer changed"


# ---- 3. op level
def scene(n1=None):
    model = make_model()
    rays = view_rays(True, orbit=25.0, frames=(1.0, 1.0, 1.0))
    boxes, _ = model._retimed_boxes(rays[0, 6:].cpu())
    model.rotation = [None, 0.6, None]
    rot = model.layer_ray_transforms(boxes)
    model.rotation = None
    return model, rays, boxes.cuda(), rot, rotated_rays(rays, *rot[1])


@pytest.mark.parametrize("n1", [12, 90, 7])                 # four samples per thread, two, the scalar kernel
@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("edits", [False, True])
def test_sample_coarse_with_one_rotated_layer(n1, replay, edits):
    _, rays, boxes, rot, turned = scene()
    jitter = torch.rand(3, N, n1, generator=torch.Generator().manual_seed(n1)).cuda() if replay else None
    kw = dict(jitter=jitter, seed=5, raw_mask=True)
    if edits:
        kw.update(edits=[(None, None), ([0.1, 0.0, 0.05], 1.2), (None, 0.9)], pivot=torch.tensor([0.0, 0.1, -0.2]))
    got = ops.sample_coarse(rays, boxes, n1, rotations=rot, **kw)
    plain = ops.sample_coarse(rays, boxes, n1, **kw)
    ref = ops.sample_coarse(turned, boxes, n1, **kw)
    for a, p, r, name in zip(got, plain, ref, ("t", "xyz", "mask")):
        assert_bit_equal(a[:, 1], r[:, 1], f"{name} of the rotated layer")
        assert_bit_equal(a[:, 0], p[:, 0], f"{name} of layer 0")
        assert_bit_equal(a[:, 2], p[:, 2], f"{name} of layer 2")
    assert not torch.equal(got[0][:, 1], plain[0][:, 1])
    assert set(got[2][:, 1].unique().tolist()) >= {1, 2}                # hits, and whole misses with their hint
    # no enabled entry: the plain call
    same = ops.sample_coarse(rays, boxes, n1, rotations=[None, None, None], **kw)
    for a, p in zip(same, plain):
        assert_bit_equal(a, p, "rotations without an entry")


@pytest.mark.parametrize("n1,n2", [(12, 6), (90, 30), (260, 8)])       # one block of 64 coarse samples, two, the unpipelined flavour
@pytest.mark.parametrize("replay", [False, True])
def test_resample_with_one_rotated_layer(n1, n2, replay):
    _, rays, boxes, rot, turned = scene()
    t, _, _ = ops.sample_coarse(rays, boxes, n1, seed=5, rotations=rot)
    g = torch.Generator().manual_seed(n1)
    weights = torch.rand(N, 3, n1, generator=g).cuda()
    u = torch.rand(3, N, n2, generator=g).cuda() if replay else None
    kw = dict(u=u, seed=5)
    got = ops.resample(t, weights, n2, rays, rotations=rot, **kw)
    plain = ops.resample(t, weights, n2, rays, **kw)
    ref = ops.resample(t, weights, n2, turned, **kw)
    for a, p, r, name in zip(got, plain, ref, ("t_fine", "xyz_fine")):
        assert_bit_equal(a[:, 1], r[:, 1], f"{name} of the rotated layer")
        assert_bit_equal(a[:, 0], p[:, 0], f"{name} of layer 0")
        assert_bit_equal(a[:, 2], p[:, 2], f"{name} of layer 2")
    assert_bit_equal(got[0], plain[0], "depths do not depend on the rotation")
    assert not torch.equal(got[1][:, 1], plain[1][:, 1])
    missed = (t[:, 1] == -1000.0).all(-1)
    assert bool(missed.any()) and bool((~missed).any())                # the all-missed shortcut's point and the general path
    # with a box edit on top
    kw.update(edits=[(None, None), ([0.1, 0.0, 0.05], 1.2), (None, 0.9)], pivot=torch.tensor([0.0, 0.1, -0.2]))
    got = ops.resample(t, weights, n2, rays, rotations=rot, **kw)
    ref = ops.resample(t, weights, n2, turned, **kw)
    assert_bit_equal(got[1][:, 1], ref[1][:, 1], "xyz_fine of the rotated, edited layer")


def test_rgb_ray_bias_and_spacenet_with_a_rotation():
    model, rays, _, rot, turned = scene()
    net = model.spacenets[0]._packed("fp32")
    dirs, times = rays[:, 3:6], rays[:, 7]
    got = ops.rgb_ray_bias(net, dirs, times, rotations=rot[1])
    ref = ops.rgb_ray_bias(net, turned[:, 3:6], times)
    assert_bit_equal(got, ref, "ray bias")
    assert_bit_equal(ops.rgb_ray_bias(net, dirs, times, rotations=[rot[1]]), ref, "ray bias, one-entry list")
    assert not torch.equal(got, ops.rgb_ray_bias(net, dirs, times))
    # on a work list: the listed rows, the others untouched (zero)
    lst = torch.arange(5, N, 3, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([lst.numel()], dtype=torch.int32, device="cuda")
    listed = ops.rgb_ray_bias(net, dirs, times, ray_list=lst, ray_count=cnt, rotations=rot[1])
    assert_bit_equal(listed[lst.long()], ref[lst.long()], "ray bias of the listed rays")
    rest = torch.ones(N, dtype=torch.bool, device="cuda")
    rest[lst.long()] = False
    assert not bool(listed[rest].any())
    # the bias network of the background takes no time
    bk = model.bkgd_spacenet._packed("fp32")
    assert_bit_equal(ops.rgb_ray_bias(bk, dirs, None, rotations=rot[1]), ops.rgb_ray_bias(bk, turned[:, 3:6], None), "ray bias, no time")
    # the network behind it, both arithmetics: only the direction of the colour branch turns
    xyz = (torch.rand(N, 5, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).cuda()
    for precision in ("fp32", "bf16x3"):
        pk = model.spacenets[0]._packed(precision)
        raw = [torch.zeros(N, 5, 4, device="cuda") for _ in range(3)]
        ops.spacenet_fwd(pk, xyz, dirs, times, raw[0], rotation=rot[1])
        ops.spacenet_fwd(pk, xyz, turned[:, 3:6], times, raw[1])
        ops.spacenet_fwd(pk, xyz, dirs, times, raw[2])
        assert_bit_equal(raw[0], raw[1], f"spacenet_fwd {precision}")
        assert_bit_equal(raw[0][..., 3], raw[2][..., 3], f"sigma {precision}")          # the density takes no direction
        assert not torch.equal(raw[0][..., :3], raw[2][..., :3])


# ---- 4. meaning: which way and about which point the layer turns
def test_a_quarter_turn_swaps_the_extents_of_layer_one():
    """Layer 1's box in the synthetic scene: x in [-1.2, -0.12], y, z in [-1, 1], centre (-0.66, 0, 0).  Turned by pi / 2 about z
    through its centre it spans x in [-1.66, 0.34], y in [-0.54, 0.54]."""
    model = make_model()
    boxes = torch.cat([model.bkgd_bbox.float(), model.bboxes[0].float()], 0)
    model.rotation = [None, math.pi / 2, None]
    rot = model.layer_ray_transforms(boxes)
    assert float((rot[1][1] - torch.tensor([-0.66, 0.0, 0.0])).abs().max()) <= 1e-6
    rays = torch.tensor([[-2.0, 0.8, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0],            # along +x through (., 0.8, 0)
                         [-2.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]]).cuda()    # along +x through the centre
    zero = torch.zeros(3, 2, 2, device="cuda")                                      # no jitter: t = near + k (far - near) / 2
    extent = lambda t: 2.0 * (t[:, 1, 1] - t[:, 1, 0])
    t0, _, m0 = ops.sample_coarse(rays, boxes.cuda(), 2, jitter=zero, raw_mask=True)
    t1, _, m1 = ops.sample_coarse(rays, boxes.cuda(), 2, jitter=zero, raw_mask=True, rotations=rot)
    assert m0[:, 1].tolist() == [1, 1] and m1[:, 1].tolist() == [2, 1]               # the off-centre ray misses the turned box
    assert t1[0, 1].tolist() == [-1000.0, -1000.0]
    assert abs(float(extent(t0)[0]) - 1.08) <= 1e-5 and abs(float(extent(t0)[1]) - 1.08) <= 1e-5
    assert abs(float(extent(t1)[1]) - 2.0) <= 1e-5
    assert abs(float(t0[1, 1, 0]) - 0.8) <= 1e-5 and abs(float(t1[1, 1, 0]) - 0.34) <= 1e-5      # entry points: x = -1.2, x = -1.66


# ---- 5. the background cache: performer rotations hit, layer 0's misses
def test_background_cache_under_a_rotation_sweep():
    model = make_model()
    K, T = syn.camera(H, W, 15.0)
    f = [1.0, 2.5, 3.0]
    rays = ops.generate_rays(K, T, H, W, frame_ids=f)

    def frame(rotation, cached):
        model.rotation = rotation
        model.view_key = view_key(K, T, H, W, f) if cached else None
        try:
            return render(model, rays)
        finally:
            model.view_key = None

    cache = stnerf_amd.BackgroundCache()
    sweep = [[None, 0.2 * k, (-0.3 * k, CENTRE)] for k in range(4)]
    want = [frame(r, False) for r in sweep]
    assert not torch.equal(want[0][0], want[1][0])
    model.set_background_cache(cache)
    for k, r in enumerate(sweep):
        got = frame(r, True)
        assert (cache.stats["hits"], cache.stats["misses"]) == (k * PIECES, PIECES), (k, cache.stats)
        for a, b in zip(got, want[k]):
            assert_bit_equal(a, b, f"cached frame {k}")
    turned_bkgd = [(0.1, CENTRE), 0.2, None]
    got = frame(turned_bkgd, True)
    assert (cache.stats["hits"], cache.stats["misses"]) == (3 * PIECES, 2 * PIECES), cache.stats
    model.set_background_cache(None)
    for a, b in zip(got, frame(turned_bkgd, False)):
        assert_bit_equal(a, b, "layer 0 rotated")


# ---- 6. the renderer's schedule
def test_render_path_follows_the_rotation_schedule():
    from stnerf_amd.render import LayeredNeuralRenderer
    from stnerf_amd.render.render_pose import render_pose
    model = make_model()
    K, T = syn.camera(H, W, 25.0)
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=2, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    r = LayeredNeuralRenderer(cfg, model=model, gt_poses=T[None], gt_Ks=[K], s_rotation=([None, 0.0, 0.4], [None, 0.8, -0.4]))
    r.set_path_fixed_gt_poses(0, 3)
    seen = []
    r.render_path(auto_save=False, on_frame=lambda idx, c, d, cl, dl: seen.append([c.clone(), d.clone()] + [x.clone() for x in cl + dl]))
    assert len(seen) == 3 and r.s_rotation_frame[1] == [None, 0.4, 0.0]
    for k in range(3):
        model.rotation = [None, 0.0 + k * 0.4, 0.4 - k * 0.4]
        c, d, cl, dl = render_pose(model, r.poses[k], r.Ks[k], H, W, r.layer_frame_pairs[k], r.far, 0, 0)
        for a, b in zip(seen[k], [c, d] + cl + dl):
            assert_bit_equal(a, b, f"frame {k}")
    assert not torch.equal(seen[0][0], seen[2][0])
    # render_pose with the renderer's own rotation= (forwarded as scale and shift are)
    r2 = LayeredNeuralRenderer(cfg, None, None, [None, 0.4, 0.0], model=model, gt_poses=T[None], gt_Ks=[K])
    c, *_ = r2.render_pose(r.poses[1], r.Ks[1], r.layer_frame_pairs[1])
    assert_bit_equal(c, seen[1][0], "rotation= of the renderer")
