"""Torch-tensor wrappers over the C ABI (one function per entry point of include/stnerf.h).

PyTorch is plumbing here: device memory, streams.  Every function launches HIP kernels from
``libstnerf_hip.so`` on the current torch stream and returns device tensors; none of them has a
PyTorch implementation to fall back to.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import torch

from stnerf_amd import hip

Tensor = torch.Tensor


def _strided_view_ptr(t: Tensor, inner: Tuple[int, ...], name: str):
    """(pointer, ray stride) of a tensor whose dim 0 is the ray and whose inner dims are dense."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if tuple(t.shape[1:]) != tuple(inner):
        raise ValueError(f"{name}: expected shape (n, {inner}), got {tuple(t.shape)}")
    expect = 1
    for d in range(t.dim() - 1, 0, -1):
        if t.shape[d] != 1 and t.stride(d) != expect:
            raise ValueError(f"{name}: inner dimensions must be dense, got strides {t.stride()}")
        expect *= t.shape[d]
    return C.c_void_p(t.data_ptr()), (t.stride(0) if t.shape[0] > 1 else expect)


def _edits(edits, pivot, l):
    """-> (LayerEdit array | None, float[3] | None).  edits: per layer (shift|None, scale|None)."""
    if edits is None:
        return None, None
    arr = (hip.LayerEdit * l)()
    for i in range(l):
        sh, sc = edits[i] if i < len(edits) else (None, None)
        if sh is not None:
            # the reference builds torch.tensor(shift[i]) (fp32), layered_rfrender.py:241,297
            v = torch.tensor(sh, dtype=torch.float32).tolist()
            arr[i].shift[0], arr[i].shift[1], arr[i].shift[2] = v
            arr[i].has_shift = 1
        if sc is not None:
            arr[i].scale = float(sc)
            arr[i].has_scale = 1
    pv = (C.c_float * 3)(*(float(x) for x in (pivot if pivot is not None else (0.0, 0.0, 0.0))))
    return arr, pv


def _rotation_struct(dst, entry):
    """Fill one hip.LayerRotation from None | (m (3,3) = R^T, centre (3,) | None): fp32 numbers as they are."""
    if entry is None:
        dst.enabled = 0
        return
    m, c = entry
    mv = torch.as_tensor(m, dtype=torch.float32).reshape(9).tolist()
    cv = [0.0, 0.0, 0.0] if c is None else torch.as_tensor(c, dtype=torch.float32).reshape(3).tolist()
    for j in range(9):
        dst.m[j] = mv[j]
    for j in range(3):
        dst.centre[j] = cv[j]
    dst.enabled = 1


def _rotations(rotations, l):
    """-> LayerRotation array of l entries | None.  rotations: per layer None | (m, centre), the pairs of
    ``LayeredRFRender.layer_ray_transforms`` (include/stnerf.h: stnerf_layer_rotation)."""
    if rotations is None or all(r is None for r in rotations):
        return None
    if len(rotations) != l:
        raise ValueError(f"rotations must have one entry per layer ({l}), got {len(rotations)}")
    arr = (hip.LayerRotation * l)()
    for i in range(l):
        _rotation_struct(arr[i], rotations[i])
    return arr


def _boxes_arg(boxes: Tensor, n: int):
    if boxes.dim() == 3:  # (l,8,3) shared
        return hip.dptr(boxes, name="boxes"), 0, boxes.shape[0]
    if boxes.dim() == 4 and boxes.shape[0] == n:  # (n,l,8,3) per ray
        return hip.dptr(boxes, name="boxes"), boxes.shape[1] * 24, boxes.shape[1]
    raise ValueError(f"boxes must be (l,8,3) or (n,l,8,3), got {tuple(boxes.shape)}")


# ---------------------------------------------------------------------------------------- a1/a2
def window_size(total: int, first: int, stripe: int, period: int) -> int:
    """Number of rays of a `total`-ray view inside the window (first, stripe, period) of include/stnerf.h."""
    if stripe <= 0:
        return max(0, total - first)
    if first >= total:
        return 0
    full, rem = divmod(total - first, period)
    return full * stripe + min(rem, stripe)


def _lens_record(lens, k: float, phase: int, points: Optional[Tensor]) -> "hip.LensRecord":
    """The stnerf_lens of an enabled ``Lens`` for one pass.  k = K^-1's [2][2]: the library's focus is a camera-space z, of k's sign.
    Without an aperture there is no table (``points`` is not read)."""
    rec = hip.LensRecord(distort=int(lens.distorts), k1=lens.k1, k2=lens.k2, k3=lens.k3, p1=lens.p1, p2=lens.p2, key=lens.key)
    if lens.aperture > 0.0:
        if points is None:
            raise ValueError("generate_rays: a lens with aperture > 0 needs lens_points=, the device table lens.table(n_points)")
        if points.dim() != 2 or points.shape[1] != 2 or points.shape[0] < 1:
            raise ValueError(f"generate_rays: lens_points must be (n_points, 2) float32, got {tuple(points.shape)}")
        rec.points = hip.dptr(points, name="lens_points").value
        rec.n_points, rec.phase, rec.decorrelate = points.shape[0], int(phase), int(lens.decorrelate)
        rec.focus = -lens.focus if k < 0 else lens.focus
    return rec


def generate_rays(K: Tensor, T: Tensor, h: int, w: int, frame_ids: Optional[Sequence[float]] = None,
                  first_ray: int = 0, n: Optional[int] = None, device="cuda", stripe: int = 0, period: int = 0,
                  pixels: Optional[Tensor] = None, offset: Sequence[float] = (0.0, 0.0), lens=None, lens_phase: int = 0,
                  lens_points: Optional[Tensor] = None) -> Tensor:
    """Rays of a view, generated on the device: (n, 6 + len(frame_ids)).  (first_ray, stripe, period) = the ray
    window of include/stnerf.h: a contiguous piece of the view (stripe = 0) or interleaved stripes.
    utils/render_helpers.py:42-128 + data/datasets/ray_dataset.py:276-281.

    ``pixels`` / ``offset`` (stnerf_generate_rays_list; progressive multi-sample frames): row i is pixel ``pixels[i]`` of the
    view -- a device int32 list naming a pixel at most once; None with ``n``: the contiguous pixels 0..n-1 -- moved by
    ``offset`` = (du, dv) pixels.  With a zero offset row i is bit-identical to row ``pixels[i]`` of the plain call.  They do
    not combine with a ray window.

    ``lens`` (stnerf_generate_rays_lens; ``stnerf_amd.lens.Lens`` or the dict of its arguments): the rays of a lens that distorts
    and / or has an aperture.  With ``lens.aperture > 0`` the ray of pass ``lens_phase`` starts at a row of ``lens_points``, the
    device (n_points, 2) float32 table ``lens.table(n_points)`` (uploaded once per frame by the caller) -- row ``lens_phase``, or
    with ``lens.decorrelate`` a row every pixel picks from its own start.  ``pixels`` / ``offset`` keep their meaning; a ray
    window does not combine with an enabled lens.  None, or a lens that changes no ray: exactly the calls above."""
    from stnerf_amd.lens import as_lens
    lens = as_lens(lens)
    lensed = lens is not None and lens.enabled
    if lensed and (first_ray or stripe or period):
        raise ValueError("generate_rays: lens= does not combine with a ray window (first_ray, stripe, period)")
    listed = pixels is not None or tuple(float(x) for x in offset) != (0.0, 0.0)
    if listed and (first_ray or stripe or period):
        raise ValueError("generate_rays: pixels= / offset= do not combine with a ray window (first_ray, stripe, period)")
    if pixels is not None:
        if pixels.dim() != 1 or (n is not None and n != pixels.shape[0]):
            raise ValueError(f"generate_rays: pixels must be a 1-D int32 list (of n entries), got {tuple(pixels.shape)} and n = {n}")
        n = pixels.shape[0]
    n = window_size(h * w, first_ray, stripe, period) if n is None else n
    kinv = torch.inverse(K.detach().to("cpu", torch.float32)).contiguous()  # :103 (torch.inverse on the host)
    Tm = torch.as_tensor(T, dtype=torch.float32).detach().cpu().contiguous()
    fids = [float(x) for x in (frame_ids or [])]
    rays = torch.empty(n, 6 + len(fids), dtype=torch.float32, device=device)
    kin = (C.c_float * 9)(*kinv.reshape(-1).tolist())
    tin = (C.c_float * 16)(*Tm.reshape(-1).tolist())
    fin = (C.c_float * max(len(fids), 1))(*(fids or [0.0]))
    if lensed:
        rec = _lens_record(lens, float(kinv[2, 2]), lens_phase, lens_points)
        hip.check(hip.lib().stnerf_generate_rays_lens(kin, tin, h, w, hip.dptr(pixels, torch.int32, "pixels"), n, float(offset[0]),
                                                      float(offset[1]), C.byref(rec), fin if fids else None, len(fids), hip.dptr(rays),
                                                      rays.shape[1], hip.stream_ptr()), "stnerf_generate_rays_lens")
        return rays
    if listed:
        hip.check(hip.lib().stnerf_generate_rays_list(kin, tin, h, w, hip.dptr(pixels, torch.int32, "pixels"), n, float(offset[0]),
                                                      float(offset[1]), fin if fids else None, len(fids), hip.dptr(rays),
                                                      rays.shape[1], hip.stream_ptr()), "stnerf_generate_rays_list")
        return rays
    hip.check(hip.lib().stnerf_generate_rays(kin, tin, h, w, first_ray, stripe, period, n, fin if fids else None, len(fids),
                                             hip.dptr(rays), rays.shape[1], hip.stream_ptr()), "stnerf_generate_rays")
    return rays


# ---------------------------------------------------------------------------------------- a5/a6
def intersect(rays: Tensor, boxes: Tensor) -> Tensor:
    """(n,l,2) = (far, near); layers/RaySamplePoint.py:8-62."""
    n = rays.shape[0]
    bp, bstride, l = _boxes_arg(boxes, n)
    out = torch.empty(n, l, 2, dtype=torch.float32, device=rays.device)
    hip.check(hip.lib().stnerf_intersect(hip.dptr(rays, name="rays"), n, rays.shape[1], bp, bstride, l,
                                         hip.dptr(out), hip.stream_ptr()), "stnerf_intersect")
    return out


def sample_coarse(rays: Tensor, boxes: Tensor, n1: int, jitter: Optional[Tensor] = None, seed: int = 0,
                  ray_index_base: int = 0, edits=None, pivot=None, want_xyz: bool = True, ray_index_stripe: int = 0,
                  ray_index_period: int = 0, raw_mask: bool = False, rotations=None):
    """-> t (n,l,n1), xyz (n,l,n1,3) | None, mask (n,l) uint8 (0 / 1 = the reference's ray_mask; with ``raw_mask`` the
    library's byte: bit 1 = the sampler's "every depth of this pair is -1000" hint, which ``composite`` accepts).
    layers/RaySamplePoint.py:70-107.  ``rotations``: per layer None | (m, centre) -- the layer sees the ray turned into its
    frame (stnerf_sample_coarse_rot)."""
    n = rays.shape[0]
    bp, bstride, l = _boxes_arg(boxes, n)
    if jitter is not None and tuple(jitter.shape) != (l, n, n1):
        raise ValueError(f"jitter must be (l,n,n1) = {(l, n, n1)}, got {tuple(jitter.shape)}")
    t = torch.empty(n, l, n1, dtype=torch.float32, device=rays.device)
    xyz = torch.empty(n, l, n1, 3, dtype=torch.float32, device=rays.device) if want_xyz else None
    mask = torch.empty(n, l, dtype=torch.uint8, device=rays.device)
    ed, pv = _edits(edits, pivot, l)
    rot = _rotations(rotations, l)
    head = (hip.dptr(rays, name="rays"), n, rays.shape[1], bp, bstride, l, n1, hip.dptr(jitter, name="jitter"), seed, ray_index_base,
            ray_index_stripe, ray_index_period, ed, pv)
    tail = (hip.dptr(t), hip.dptr(xyz), hip.dptr(mask, torch.uint8), hip.stream_ptr())
    if rot is None:
        hip.check(hip.lib().stnerf_sample_coarse(*head, *tail), "stnerf_sample_coarse")
    else:
        hip.check(hip.lib().stnerf_sample_coarse_rot(*head, rot, *tail), "stnerf_sample_coarse_rot")
    return t, xyz, (mask if raw_mask else mask.bitwise_and_(1))


def compact_rays(mask: Tensor):
    """-> ray_list (l,n) int32, ray_count (l,) int32 (device; no host sync)."""
    n, l = mask.shape
    ray_list = torch.empty(l, n, dtype=torch.int32, device=mask.device)
    ray_count = torch.zeros(l, dtype=torch.int32, device=mask.device)
    hip.check(hip.lib().stnerf_compact_rays(hip.dptr(mask, torch.uint8, "mask"), n, l,
                                            hip.dptr(ray_list, torch.int32), hip.dptr(ray_count, torch.int32),
                                            hip.stream_ptr()), "stnerf_compact_rays")
    return ray_list, ray_count


# ---------------------------------------------------------------------------------------- networks
SPACENET_KEYS = ["stage1.0", "stage1.2", "stage1.4", "stage1.6", "stage2.0", "stage2.2", "stage2.4",
                 "density_net.0", "rgb_net.1", "rgb_net.3"]
MOTIONNET_KEYS = [f"motion_net.{j}" for j in (0, 2, 4, 6, 8, 10)]


PRECISIONS = ("bf16x3", "fp32")   # the library default first


class PackedNet:
    """Kernel-layout weights of one network, resident on the device."""

    def __init__(self, kind: int, blob: Tensor, precision: str = "fp32"):
        self.kind, self.blob, self.precision = kind, blob, precision

    @property
    def use_time(self) -> bool:
        return self.kind in (hip.NET_SPACE_TIME, hip.NET_SPACE_TIME_DEEP)


_PACK_CHECK = [True]


class training_pack:
    """Context of the packs a training step makes (modeling/autograd.py): no finiteness check -- no synchronisation -- in the device bf16x3 packer."""

    def __enter__(self):
        self.prev, _PACK_CHECK[0] = _PACK_CHECK[0], False

    def __exit__(self, *exc):
        _PACK_CHECK[0] = self.prev


def pack_net(kind: int, weights: List[Tensor], biases: List[Tensor], device="cuda", precision: str = "fp32") -> PackedNet:
    """Repack reference-layout nn.Linear tensors (host copy) and upload.  precision: "fp32" (exact f32 MFMA) or "bf16x3"
    (three bf16 pieces per operand, six MFMAs, two accumulators: the full fp32 significand and exponent range; the stage
    kernel only)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    lib = hip.lib()
    size_fn = {"fp32": lib.stnerf_packed_bytes, "bf16x3": lib.stnerf_packed_bytes_bf16x3}[precision]
    pack_fn = {"fp32": lib.stnerf_pack_net, "bf16x3": lib.stnerf_pack_net_bf16x3}[precision]
    nbytes = size_fn(kind)
    if nbytes < 0:
        hip.check(int(nbytes), "stnerf_packed_bytes")
    if all(t.is_cuda for t in list(weights) + list(biases)) and not (precision == "bf16x3" and os.environ.get("STNERF_PACK_BF16X3_HOST") == "1"):
        # tensors that live on the GPU are packed there (stnerf_pack_net_device / stnerf_pack_net_bf16x3_device: the same blobs bit for
        # bit): no D2H / CPU loop / H2D per network -- a training loop repacks after every optimizer.step().  (The bf16x3 device packer
        # does not refuse non-finite weights the way the host packer does: STNERF_PACK_BF16X3_HOST=1 keeps the host path.)
        dev = weights[0].device
        ws = [w.detach().to(torch.float32).contiguous() for w in weights]
        bs = [b.detach().to(torch.float32).contiguous() for b in biases]
        wp = (C.c_void_p * len(ws))(*(w.data_ptr() for w in ws))
        bp = (C.c_void_p * len(bs))(*(b.data_ptr() for b in bs))
        if precision == "fp32":
            blob = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            fn, name = lib.stnerf_pack_net_device, "stnerf_pack_net_device"
        else:       # (the stage kernel streams it by 16-byte LDS-DMA from 1 KB-aligned sections)
            # The host packer refuses what cannot be split into three bf16 pieces (NaN, inf, |w| > 3.3895e38: include/stnerf.h).  Packing on
            # the device, the same refusal costs a host <- device synchronisation: paid where a model is packed to RENDER (once per weight
            # version), not inside a training step (``training_pack()``, modeling/autograd.py: the step would wait for the GPU after every
            # optimizer.step(); a non-finite weight there gives NaN outputs and a NaN loss).
            if _PACK_CHECK[0]:
                worst = float(torch.stack([t.abs().max() if t.numel() else t.new_zeros(()) for t in ws + bs]).nan_to_num(nan=float("inf")).max())
                if not worst <= 3.3895313892515355e38:
                    raise ValueError(f"stnerf_pack_net_bf16x3_device: a weight or bias is not finite or exceeds bf16's range (|w| <= 3.3895e38): "
                                     f"{worst:g} -- use the exact-f32 packing (precision='fp32') for such a network")
            raw = torch.empty(nbytes + 1024, dtype=torch.uint8, device=dev)
            off = (-raw.data_ptr()) % 1024
            blob = raw[off:off + nbytes].view(torch.float32)
            fn, name = lib.stnerf_pack_net_bf16x3_device, "stnerf_pack_net_bf16x3_device"
        with torch.cuda.device(dev):
            hip.check(fn(kind, wp, bp, len(ws), hip.dptr(blob), nbytes, hip.stream_ptr()), name)
        return PackedNet(kind, blob, precision)
    ws = [w.detach().to("cpu", torch.float32).contiguous() for w in weights]
    bs = [b.detach().to("cpu", torch.float32).contiguous() for b in biases]
    host = torch.empty(nbytes // 4, dtype=torch.float32)
    wp = (C.c_void_p * len(ws))(*(w.data_ptr() for w in ws))
    bp = (C.c_void_p * len(bs))(*(b.data_ptr() for b in bs))
    hip.check(pack_fn(kind, wp, bp, len(ws), C.c_void_p(host.data_ptr()), nbytes), "stnerf_pack_net")
    blob = host.to(device)
    if precision == "bf16x3" and blob.data_ptr() % 1024:   # (the stage kernel streams it by 16-byte LDS-DMA from 1 KB-aligned sections)
        raw = torch.empty(nbytes + 1024, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 1024
        blob = raw[off:off + nbytes].view(torch.float32)
        blob.copy_(host)
    return PackedNet(kind, blob, precision)


def _pe_columns(w: Tensor, dim: int, n_freq: int, include_input: bool, present: bool = True) -> Tensor:
    """Columns of a Linear weight that multiply one positional-encoding block, widened to the kernels' layout
    [x, sin, cos, ...] (dim*(1+2L) columns).  The kernels always build that block; an encoding without the raw
    input (TKERNEL_INC_RAW=False, utils/dimension_kernel.py:12-14) or an absent direction encoding (USE_DIR=False,
    modeling/spacenet.py:22-31) gets ZERO weight columns there, which leaves every output bit-identical."""
    full = dim * (1 + 2 * n_freq)
    if not present:
        return w.new_zeros(w.shape[0], full)
    if include_input:
        assert w.shape[1] == full
        return w
    assert w.shape[1] == full - dim
    return torch.cat([w.new_zeros(w.shape[0], dim), w], 1)


def pack_spacenet(state: dict, prefix: str, device="cuda", precision: str = "fp32") -> PackedNet:
    """From reference state_dict keys ``{prefix}.stage1.0.weight`` ....  The SpaceNet flavour
    (use_time, use_dir, include_input, deep_rgb: modeling/spacenet.py:16-86) is read off the tensor shapes."""
    deep = f"{prefix}.rgb_net.7.weight" in state          # deep_rgb: rgb_net.{1,3,5,7} (modeling/spacenet.py:68-79)
    keys = SPACENET_KEYS + (["rgb_net.5", "rgb_net.7"] if deep else [])
    on_device = all(state[f"{prefix}.{k}.weight"].is_cuda for k in keys)     # (packed where they live, either arithmetic: pack_net)
    ws = [state[f"{prefix}.{k}.weight"].detach().float() if on_device else state[f"{prefix}.{k}.weight"].detach().float().cpu() for k in keys]
    bs = [state[f"{prefix}.{k}.bias"] for k in keys]
    pos_w = ws[0].shape[1]
    if pos_w not in (63, 60):
        raise ValueError(f"{prefix}.stage1.0 has in-width {pos_w}: only c_pos=3 with PE_10 is supported")
    inc = pos_w == 63
    dir_w, time_w = (27, 21) if inc else (24, 20)
    extra = ws[8].shape[1] - 256
    flavours = {dir_w + time_w: (True, True), dir_w: (True, False), time_w: (False, True), 0: (False, False)}
    if extra not in flavours:
        raise ValueError(f"{prefix}.rgb_net.1 has in-width {ws[8].shape[1]}: not a SpaceNet colour head")
    use_dir, use_time = flavours[extra]
    ws[0] = _pe_columns(ws[0], 3, 10, inc)
    ws[4] = torch.cat([ws[4][:, :256], _pe_columns(ws[4][:, 256:], 3, 10, inc)], 1)
    r = ws[8]
    parts = [r[:, :256], _pe_columns(r[:, 256:256 + (dir_w if use_dir else 0)], 3, 4, inc, use_dir)]
    if use_time:
        parts.append(_pe_columns(r[:, 256 + (dir_w if use_dir else 0):], 1, 10, inc))
    ws[8] = torch.cat(parts, 1)
    kind = ((hip.NET_SPACE_TIME_DEEP if deep else hip.NET_SPACE_TIME) if use_time
            else (hip.NET_SPACE_DEEP if deep else hip.NET_SPACE))
    return pack_net(kind, ws, bs, device, precision)


def pack_motionnet(state: dict, prefix: str, device="cuda", precision: str = "fp32") -> PackedNet:
    on_device = all(state[f"{prefix}.{k}.weight"].is_cuda for k in MOTIONNET_KEYS)
    ws = [state[f"{prefix}.{k}.weight"].detach().float() if on_device else state[f"{prefix}.{k}.weight"].detach().float().cpu() for k in MOTIONNET_KEYS]
    bs = [state[f"{prefix}.{k}.bias"] for k in MOTIONNET_KEYS]
    if ws[0].shape[1] not in (84, 80):
        raise ValueError(f"{prefix}.motion_net.0 has in-width {ws[0].shape[1]}: only c_input=4 with PE_10 is supported")
    ws[0] = _pe_columns(ws[0], 4, 10, ws[0].shape[1] == 84)
    return pack_net(hip.NET_MOTION, ws, bs, device, precision)


PROFILE_KERNELS = ("spacenet", "motionnet", "composite", "resample", "sample_coarse", "mlp_stage", "copy_layer_raw", "occupancy_cull",
                   "occupancy_build", "occupancy_rows", "ray_stop", "visibility_rows", "background_rows", "copy_layer_raw_listed",
                   "scene_occluder", "occluder_stop", "deep_count", "deep_offsets", "deep_fill", "deep_composite",
                   "proposal_density")


def profile_begin() -> None:
    """Start the library's launch profiler (HIP events on the launch stream around every kernel launch)."""
    hip.check(hip.lib().stnerf_profile_begin(), "stnerf_profile_begin")


def profile_end():
    """Stop profiling; -> list of dicts (kernel name, kind, n_rays, ns, tag, bytes_per_ray, ms) in launch order."""
    n = C.c_int(0)
    hip.check(hip.lib().stnerf_profile_end(None, 0, C.byref(n)), "stnerf_profile_end")
    if n.value == 0:
        return []
    buf = (hip.ProfileRecord * n.value)()
    hip.check(hip.lib().stnerf_profile_end(buf, n.value, C.byref(n)), "stnerf_profile_end")
    return [dict(kernel=PROFILE_KERNELS[r.kernel], kind=r.kind, n_rays=r.n_rays, ns=r.ns, tag=r.tag,
                 bytes_per_ray=r.bytes_per_ray, ms=r.ms) for r in buf]


def _worklist(ray_list, ray_count):
    return hip.dptr(ray_list, torch.int32, "ray_list"), hip.dptr(ray_count, torch.int32, "ray_count")


def spacenet_fwd(net: PackedNet, xyz: Tensor, dirs: Tensor, times: Optional[Tensor], raw: Tensor,
                 ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None, rotation=None) -> Tensor:
    """xyz (n,ns,3), dirs (n,3), times (n,) | None, raw (n,ns,4) out; all may be strided views whose
    dim 0 is the ray.  Writes raw {r,g,b,sigma} for the listed rays.  modeling/spacenet.py:101-160.
    ``rotation``: None | (m, centre) of the net's layer -- the colour branch encodes m @ dir (stnerf_spacenet_fwd_rot)."""
    n, ns = xyz.shape[0], xyz.shape[1]
    if net.use_time and times is None:
        raise ValueError("this SpaceNet takes time: pass times (n,)")
    if net.precision == "bf16x3":   # the split-bf16 arithmetic exists as the stage kernel: a one-layer stage
        mlp_stage([dict(space=net, motion=None, xyz=xyz, raw=raw, times=times if net.use_time else None, ray_list=ray_list,
                        ray_count=ray_count, rotation=rotation)], dirs, ns, deep_rgb=net.kind in (hip.NET_SPACE_DEEP, hip.NET_SPACE_TIME_DEEP))
        return raw
    xp, xs = _strided_view_ptr(xyz, (ns, 3), "xyz")
    dp, ds = _strided_view_ptr(dirs, (3,), "dirs")
    rp, rs = _strided_view_ptr(raw, (ns, 4), "raw")
    if net.use_time:
        tp, ts = _strided_view_ptr(times.reshape(n), (), "times")
    else:
        tp, ts = C.c_void_p(0), 0
    lp, cp = _worklist(ray_list, ray_count)
    # workspace of the per-ray part of rgb_net.1 (stnerf_rgb_ray_bias): one row of 128 floats per ray
    ray_bias = torch.empty(n, 128, dtype=torch.float32, device=raw.device)
    if rotation is None:
        hip.check(hip.lib().stnerf_spacenet_fwd(net.kind, hip.dptr(net.blob), n, ns, lp, cp, xp, xs, dp, ds, tp, ts, rp, rs,
                                                hip.dptr(ray_bias), hip.stream_ptr()), "stnerf_spacenet_fwd")
    else:
        rot = _rotations([rotation], 1)
        hip.check(hip.lib().stnerf_spacenet_fwd_rot(net.kind, hip.dptr(net.blob), n, ns, lp, cp, xp, xs, dp, ds, tp, ts, rp, rs,
                                                    hip.dptr(ray_bias), rot, hip.stream_ptr()), "stnerf_spacenet_fwd_rot")
    return raw


def rgb_ray_bias(net: PackedNet, dirs: Tensor, times: Optional[Tensor], ray_list: Optional[Tensor] = None,
                 ray_count: Optional[Tensor] = None, rotations=None) -> Tensor:
    """The per-ray part of rgb_net.1 (stnerf_rgb_ray_bias): (n, 128) = bias + W[:, 256:] relu([PE_4(dir), PE_10(time)]) for
    the listed rays (other rows are zero here).  modeling/spacenet.py:80-86,141-151.  ``rotations``: None, one (m, centre)
    pair or a one-entry list of them -- the net's layer is rotated and m @ dir is encoded (stnerf_rgb_ray_bias_rot)."""
    n = dirs.shape[0]
    if net.precision != "fp32":
        raise ValueError("stnerf_rgb_ray_bias reads the exact-f32 blob layout: pack the network 'fp32' for this call "
                         f"(got a {net.precision!r} blob)")
    dp, ds = _strided_view_ptr(dirs, (3,), "dirs")
    if net.use_time:
        if times is None:
            raise ValueError("this SpaceNet takes time: pass times (n,)")
        tp, ts = _strided_view_ptr(times.reshape(n), (), "times")
    else:
        tp, ts = C.c_void_p(0), 0
    lp, cp = _worklist(ray_list, ray_count)
    out = torch.zeros(n, 128, dtype=torch.float32, device=dirs.device)
    if isinstance(rotations, list):
        if len(rotations) != 1:
            raise ValueError(f"rgb_ray_bias works on one layer: rotations must be one (m, centre) pair, got {len(rotations)} entries")
        rotations = rotations[0]
    if rotations is None:
        hip.check(hip.lib().stnerf_rgb_ray_bias(net.kind, hip.dptr(net.blob), n, lp, cp, dp, ds, tp, ts, hip.dptr(out),
                                                hip.stream_ptr()), "stnerf_rgb_ray_bias")
    else:
        hip.check(hip.lib().stnerf_rgb_ray_bias_rot(net.kind, hip.dptr(net.blob), n, lp, cp, dp, ds, tp, ts, hip.dptr(out),
                                                    _rotations([rotations], 1), hip.stream_ptr()), "stnerf_rgb_ray_bias_rot")
    return out


def motionnet_fwd(net: PackedNet, xyz: Tensor, times: Tensor, flow: Optional[Tensor] = None,
                  add_to_xyz: bool = True, ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None,
                  plain_time: bool = False):
    """xyz (n,ns,3) (updated in place if add_to_xyz), times (n,), flow (n,ns,3) out | None.
    modeling/motion_net.py:34-71 + layered_rfrender.py:355-356.  plain_time = MotionNet(input_time=False):
    the time column is encoded as given instead of lerping the encodings of floor(t) and floor(t)+1."""
    n, ns = xyz.shape[0], xyz.shape[1]
    if net.precision == "bf16x3":
        raise ValueError("a bf16x3 MotionNet runs fused in front of its SpaceNet (ops.mlp_stage); there is no stand-alone "
                         "launch -- pack it 'fp32' for the op-level call")
    xp, xs = _strided_view_ptr(xyz, (ns, 3), "xyz")
    tp, ts = _strided_view_ptr(times.reshape(n), (), "times")
    if flow is not None:
        fp, fs = _strided_view_ptr(flow, (ns, 3), "flow")
    else:
        fp, fs = C.c_void_p(0), 0
    lp, cp = _worklist(ray_list, ray_count)
    flags = (hip.MOTION_ADD_TO_XYZ if add_to_xyz else 0) | (hip.MOTION_PLAIN_TIME if plain_time else 0)
    hip.check(hip.lib().stnerf_motionnet_fwd(hip.dptr(net.blob), n, ns, lp, cp, xp, xs, tp, ts, fp, fs, flags,
                                             hip.stream_ptr()), "stnerf_motionnet_fwd")
    return flow


def mlp_stage(layers: Sequence[dict], dirs: Tensor, ns: int, deep_rgb: bool = False, sigmoid_rgb: bool = False) -> None:
    """One persistent launch over every listed layer (stnerf_mlp_stage).  Each dict: space (PackedNet), motion
    (PackedNet | None), xyz (n,ns,3), raw (n,ns,4) out, times (n,) | None, ray_list / ray_count | None,
    plain_time (bool), rotation (None | (m, centre): the layer's ray-bias launch encodes m @ dir).  Views may be strided as long as all layers share the ray strides.  The arithmetic follows the
    nets' packing: all "fp32" (exact f32 MFMA) or all "bf16x3" (split-bf16 MFMA).
    row_list / row_count (int32 device tensors | None, both or neither): the layer's rows are the first ``row_count`` words
    ``ray << 8 | k`` of ``row_list`` (``occupancy_rows`` writes them) instead of ray_count x ns; a sample on no list is not
    written.  With a list on any layer the launch is stnerf_mlp_stage_rows' row-list flavour of the kernel."""
    n = dirs.shape[0]
    arr = (hip.StageLayer * len(layers))()
    rows = (hip.StageRows * len(layers))()
    listed = False
    rots = (hip.LayerRotation * len(layers))()       # (outlives the call below)
    strides = None
    precs = set()
    dp, ds = _strided_view_ptr(dirs, (3,), "dirs")
    for i, ly in enumerate(layers):
        xp, xs = _strided_view_ptr(ly["xyz"], (ns, 3), "xyz")
        rp, rs = _strided_view_ptr(ly["raw"], (ns, 4), "raw")
        tp, ts = (_strided_view_ptr(ly["times"].reshape(n), (), "times") if ly.get("times") is not None else (C.c_void_p(0), 0))
        if strides is None:
            strides = [xs, rs, ts]
        if ts and not strides[2]:
            strides[2] = ts
        if (xs, rs) != tuple(strides[:2]) or (ts and ts != strides[2]):
            raise ValueError("mlp_stage: every layer must share the xyz / raw / times ray strides")
        precs.add(ly["space"].precision)
        if ly.get("motion") is not None:
            precs.add(ly["motion"].precision)
        lp, cp = _worklist(ly.get("ray_list"), ly.get("ray_count"))
        a = arr[i]
        a.space, a.motion = ly["space"].blob.data_ptr(), (ly["motion"].blob.data_ptr() if ly.get("motion") is not None else None)
        a.ray_list, a.ray_count, a.xyz, a.raw, a.times = lp.value, cp.value, xp.value, rp.value, tp.value
        a.use_time, a.motion_flags = int(ly["space"].use_time), (hip.MOTION_PLAIN_TIME if ly.get("plain_time") else 0)
        if ly.get("rotation") is not None:
            _rotation_struct(rots[i], ly["rotation"])
            a.rotation = C.pointer(rots[i])
        if (ly.get("row_list") is None) != (ly.get("row_count") is None):
            raise ValueError("mlp_stage: a layer's row_list and row_count go together")
        if ly.get("row_list") is not None:
            rows[i].row_list = hip.dptr(ly["row_list"], torch.int32, "row_list").value
            rows[i].row_count = hip.dptr(ly["row_count"], torch.int32, "row_count").value
            listed = True
    if precs not in ({"fp32"}, {"bf16x3"}):
        raise ValueError(f"mlp_stage: every network of a launch must be packed 'fp32' or every one 'bf16x3' (got {sorted(precs)})")
    bx = 4 if precs == {"bf16x3"} else 0
    queue = torch.zeros(1, dtype=torch.int32, device=dirs.device)
    ray_bias = torch.empty(len(layers), n, 128, dtype=torch.float32, device=dirs.device)   # rgb_net.1 per ray (stnerf_rgb_ray_bias)
    flags = (1 if deep_rgb else 0) | (2 if sigmoid_rgb else 0) | bx
    if listed:
        hip.check(hip.lib().stnerf_mlp_stage_rows(arr, rows, len(layers), n, ns, dp, ds, strides[2], strides[0], strides[1], flags,
                                                  C.c_void_p(queue.data_ptr()), hip.dptr(ray_bias), hip.stream_ptr()), "stnerf_mlp_stage_rows")
        return
    hip.check(hip.lib().stnerf_mlp_stage(arr, len(layers), n, ns, dp, ds, strides[2], strides[0], strides[1], flags,
                                         C.c_void_p(queue.data_ptr()), hip.dptr(ray_bias), hip.stream_ptr()), "stnerf_mlp_stage")


def encode(x: Tensor, n_freq: int, include_input: bool = True) -> Tensor:
    """Positional encoding of x (..., dim) -> (..., dim*(include_input + 2*n_freq)); utils/dimension_kernel.py:3-73."""
    dim = x.shape[-1]
    flat = x.reshape(-1, dim).contiguous()
    y = torch.empty(flat.shape[0], dim * (int(include_input) + 2 * n_freq), dtype=torch.float32, device=x.device)
    hip.check(hip.lib().stnerf_encode(hip.dptr(flat, name="x"), flat.shape[0], dim, n_freq, int(include_input),
                                      hip.dptr(y), hip.stream_ptr()), "stnerf_encode")
    return y.reshape(*x.shape[:-1], y.shape[-1])


def gen_weight(sigma: Tensor, delta: Tensor) -> Tensor:
    """sigma (n,S) raw, delta (n,S) -> weights (n,S); layers/render_layer.py:8-17."""
    n, S = delta.shape
    sg = sigma.reshape(n, S).contiguous()
    w = torch.empty(n, S, dtype=torch.float32, device=delta.device)
    hip.check(hip.lib().stnerf_gen_weight(hip.dptr(sg, name="sigma"), hip.dptr(delta.contiguous(), name="delta"), n, S,
                                          hip.dptr(w), hip.stream_ptr()), "stnerf_gen_weight")
    return w


# ---------------------------------------------------------------------------------------- a10-a13
def composite_params(border: float = 1e10, near: float = 0.0, fine: bool = False, cut_negative_t: bool = False,
                     thresholds: Optional[Sequence[Optional[float]]] = None, sigma_scale: Optional[Sequence[float]] = None,
                     evaluated: Optional[Sequence[int]] = None, rgb_activated: bool = False) -> "hip.CompositeParams":
    """The stnerf_composite_params of a stage (include/stnerf.h): shared by ``composite`` and ``composite_bwd``."""
    p = hip.CompositeParams()
    p.border, p.near, p.fine, p.cut_negative_t = border, near, int(fine), int(cut_negative_t)
    p.rgb_activated = int(rgb_activated)
    for i in range(hip.MAX_LAYERS):
        th = thresholds[i] if thresholds is not None and i < len(thresholds) else None
        p.threshold[i] = 0.0 if th is None else float(th)
        p.use_threshold[i] = 0 if th is None else 1
        p.sigma_scale[i] = float(sigma_scale[i]) if sigma_scale is not None and i < len(sigma_scale) else 1.0
        p.evaluated[i] = int(evaluated[i]) if evaluated is not None and i < len(evaluated) else 1
    return p


def composite(t: Tensor, raw: Tensor, mask: Optional[Tensor], border: float = 1e10, near: float = 0.0,
              fine: bool = False, cut_negative_t: bool = False, thresholds: Optional[Sequence[Optional[float]]] = None,
              sigma_scale: Optional[Sequence[float]] = None, evaluated: Optional[Sequence[int]] = None,
              want_weights: bool = False, want_order: bool = False, rgb_activated: bool = False, two_pass: bool = True,
              params: Optional["hip.CompositeParams"] = None):
    """t (n,l,S), raw (n,l,S,4), mask (n,l) uint8 | None ->
    layer_out (n,l,5), mixed_out (n,5), weights (n,l,S) | None, order (n,l*S) int32 | None.
    layers/render_layer.py:8-58 + modeling/layered_rfrender.py:414-448 / :538-606.
    evaluated[i]: 0 = hidden layer, 1 = evaluated where mask is set, 2 = evaluated on every ray (the background)."""
    n, l, S = t.shape
    p = params if params is not None else composite_params(border, near, fine, cut_negative_t, thresholds, sigma_scale, evaluated,
                                                           rgb_activated)
    layer_out = torch.empty(n, l, 5, dtype=torch.float32, device=t.device)
    mixed_out = torch.empty(n, 5, dtype=torch.float32, device=t.device)
    weights = torch.empty(n, l, S, dtype=torch.float32, device=t.device) if want_weights else None
    order = torch.empty(n, l * S, dtype=torch.int32, device=t.device) if want_order else None
    scratch = torch.empty(n, dtype=torch.uint8, device=t.device) if two_pass else None   # single-layer rays first (see the header)
    hip.check(hip.lib().stnerf_composite(hip.dptr(t, name="t"), hip.dptr(raw, name="raw"),
                                         hip.dptr(mask, torch.uint8, "mask"), n, l, S, C.byref(p), hip.dptr(layer_out),
                                         hip.dptr(mixed_out), hip.dptr(weights), hip.dptr(order, torch.int32),
                                         hip.dptr(scratch, torch.uint8), hip.stream_ptr()), "stnerf_composite")
    return layer_out, mixed_out, weights, order


def composite_scene(t: Tensor, raw: Tensor, mask: Optional[Tensor], border: float = 1e10, near: float = 0.0,
                    fine: bool = False, cut_negative_t: bool = False, thresholds: Optional[Sequence[Optional[float]]] = None,
                    sigma_scale: Optional[Sequence[float]] = None, evaluated: Optional[Sequence[int]] = None,
                    want_weights: bool = False, want_order: bool = False, rgb_activated: bool = False, two_pass: bool = True,
                    params: Optional["hip.CompositeParams"] = None):
    """``composite`` with the in-scene layer passes (stnerf_composite_scene) ->
    layer_out (n,l,5), mixed_out (n,5), weights (n,l,S) | None, merged_weights (n,l,S), scene (n,l,5).
    merged_weights: every sample's weight in the MIXED composite, at its source index; scene[:, i] = layer i's share of the mixed
    image {premultiplied colour(3), weighted depth, alpha}, occluded by and occluding the others.  sum_i scene[:, i] = mixed_out up
    to fp32 summation order.  ``want_order`` selects the LDS-staged route, as in ``composite`` (the order itself is not returned)."""
    n, l, S = t.shape
    p = params if params is not None else composite_params(border, near, fine, cut_negative_t, thresholds, sigma_scale, evaluated,
                                                           rgb_activated)
    dev = t.device
    layer_out = torch.empty(n, l, 5, dtype=torch.float32, device=dev)
    mixed_out = torch.empty(n, 5, dtype=torch.float32, device=dev)
    weights = torch.empty(n, l, S, dtype=torch.float32, device=dev) if want_weights else None
    order = torch.empty(n, l * S, dtype=torch.int32, device=dev) if want_order else None
    scratch = torch.empty(n, dtype=torch.uint8, device=dev) if two_pass else None
    merged = torch.empty(n, l, S, dtype=torch.float32, device=dev)
    scene = torch.empty(n, l, 5, dtype=torch.float32, device=dev)
    hip.check(hip.lib().stnerf_composite_scene(hip.dptr(t, name="t"), hip.dptr(raw, name="raw"),
                                               hip.dptr(mask, torch.uint8, "mask"), n, l, S, C.byref(p), hip.dptr(layer_out),
                                               hip.dptr(mixed_out), hip.dptr(weights), hip.dptr(order, torch.int32),
                                               hip.dptr(scratch, torch.uint8), hip.dptr(merged), hip.dptr(scene),
                                               hip.stream_ptr()), "stnerf_composite_scene")
    return layer_out, mixed_out, weights, merged, scene


def composite_bwd(t: Tensor, raw: Tensor, mask: Optional[Tensor], order: Optional[Tensor], params: "hip.CompositeParams",
                  g_layer: Optional[Tensor], g_mixed: Optional[Tensor]) -> Tensor:
    """dLoss/d raw (n,l,S,4) from dLoss/d layer_out (n,l,5) and dLoss/d mixed_out (n,5) (either may be None):
    stnerf_composite_bwd, the backward of ``composite`` called with the same t / raw / mask / params (order: its output)."""
    n, l, S = t.shape
    d_raw = torch.empty(n, l, S, 4, dtype=torch.float32, device=t.device)
    if n == 0:                                                         # (an empty tensor has no device pointer to hand over)
        return d_raw
    hip.check(hip.lib().stnerf_composite_bwd(hip.dptr(t, name="t"), hip.dptr(raw, name="raw"), hip.dptr(mask, torch.uint8, "mask"),
                                             hip.dptr(order, torch.int32, "order"), n, l, S, C.byref(params),
                                             hip.dptr(g_layer, name="g_layer"), hip.dptr(g_mixed, name="g_mixed"), hip.dptr(d_raw),
                                             hip.stream_ptr()), "stnerf_composite_bwd")
    return d_raw


def resample(t: Tensor, weights: Tensor, n2: int, rays: Tensor, u: Optional[Tensor] = None, seed: int = 0,
             ray_index_base: int = 0, edits=None, pivot=None, want_xyz: bool = True, debug: bool = False,
             ray_index_stripe: int = 0, ray_index_period: int = 0, mask: Optional[Tensor] = None, rotations=None):
    """t (n,l,n1), weights (n,l,n1) -> t_fine (n,l,n1+n2) ascending, xyz_fine (n,l,n1+n2,3) | None
    [, z_new (n,l,n2), inds (n,l,n2) int32, cdf (n,l,n1-1) if debug].
    utils/sample_pdf.py:18-63 + modeling/layered_rfrender.py:459-475.  ``mask`` (n,l) uint8 with the sampler's hints
    (``sample_coarse(raw_mask=True)``): pairs flagged "missed" are skipped, their output rows stay unwritten.
    ``rotations``: per layer None | (m, centre) -- a rotated layer's points are those of the turned ray (stnerf_resample_rot)."""
    n, l, n1 = t.shape
    if u is not None and tuple(u.shape) != (l, n, n2):
        raise ValueError(f"u must be (l,n,n2) = {(l, n, n2)}, got {tuple(u.shape)}")
    dev = t.device
    t_fine = torch.empty(n, l, n1 + n2, dtype=torch.float32, device=dev)
    xyz = torch.empty(n, l, n1 + n2, 3, dtype=torch.float32, device=dev) if want_xyz else None
    z_new = torch.empty(n, l, n2, dtype=torch.float32, device=dev) if debug else None
    inds = torch.empty(n, l, n2, dtype=torch.int32, device=dev) if debug else None
    cdf = torch.empty(n, l, n1 - 1, dtype=torch.float32, device=dev) if debug else None
    ed, pv = _edits(edits, pivot, l)
    rot = _rotations(rotations, l)
    head = (hip.dptr(t, name="t"), hip.dptr(weights, name="weights"), n, l, n1, n2, hip.dptr(u, name="u"), seed, ray_index_base,
            ray_index_stripe, ray_index_period, hip.dptr(rays, name="rays"), rays.shape[1], ed, pv)
    tail = (hip.dptr(mask, torch.uint8, "mask"), hip.dptr(t_fine), hip.dptr(xyz), hip.dptr(z_new), hip.dptr(inds, torch.int32),
            hip.dptr(cdf), hip.stream_ptr())
    if rot is None:
        hip.check(hip.lib().stnerf_resample(*head, *tail), "stnerf_resample")
    else:
        hip.check(hip.lib().stnerf_resample_rot(*head, rot, *tail), "stnerf_resample_rot")
    if debug:
        return t_fine, xyz, z_new, inds, cdf
    return t_fine, xyz


# ---------------------------------------------------------------------------------------- whole pipeline
def fill_edits(dst, edits, l):
    """Copy per-layer (shift|None, scale|None) pairs into a LayerEdit array field of RenderParams."""
    for i in range(l):
        sh, sc = edits[i] if (edits is not None and i < len(edits)) else (None, None)
        dst[i].has_shift, dst[i].has_scale, dst[i].scale = 0, 0, 1.0
        if sh is not None:
            v = torch.tensor(sh, dtype=torch.float32).tolist()   # fp32, as torch.tensor(shift[i]) in the reference
            dst[i].shift[0], dst[i].shift[1], dst[i].shift[2] = v
            dst[i].has_shift = 1
        if sc is not None:
            dst[i].scale, dst[i].has_scale = float(sc), 1


def _layer_flags(flags, l, name):
    if len(flags) != l:
        raise ValueError(f"{name} must have one entry per layer ({l}), got {len(flags)}")
    return (C.c_int32 * l)(*(int(bool(f)) for f in flags))


# (the size query reads only whether a background grid has bits: any non-null pointer stands for "a grid will be given")
_SOME_GRID = (hip.Occupancy * 1)()
_SOME_GRID[0].bits = C.addressof(_SOME_GRID)


def render_workspace_bytes(n: int, l: int, n1: int, n2: int, only_coarse: bool, occupancy_samples=None, terminate=None,
                           background: bool = False, background_rays: bool = False) -> int:
    """Bytes of ``render_rays``'s workspace.  ``occupancy_samples``: the per-layer flags of the sample cull or None -- only
    with a flag set does the workspace grow, by the flagged layers' row lists (stnerf_render_workspace_bytes_samples).
    ``terminate``: the per-layer flags of early ray termination or None -- with a flag set (and a fine stage) the workspace grows
    by the stop depths and the flagged layers' fine row lists (stnerf_render_workspace_bytes_terminated).
    ``background``: a background grid will be given -- the workspace grows by layer 0's row list unless termination has given it one
    (stnerf_render_workspace_bytes_background).  ``background_rays``: a per-ray background mask will be given -- the same growth
    (the query reads only whether stnerf_render_options.bkgd_rays is set)."""
    opts = hip.RenderOptions()
    if background_rays:
        opts.bkgd_rays = C.addressof(_SOME_GRID)
    if occupancy_samples is not None and any(occupancy_samples):
        opts.samples = _layer_flags(occupancy_samples, l, "occupancy_samples")
    if terminate is not None:
        opts.terminate = _layer_flags(terminate, l, "terminate")
    if background:
        opts.bkgd_grid = _SOME_GRID
    nb = hip.lib().stnerf_render_workspace_bytes_opts(n, l, n1, n2, int(only_coarse), C.byref(opts))
    if nb < 0:
        hip.check(int(nb), "stnerf_render_workspace_bytes")
    return int(nb)


def copy_layer_raw(raw: Tensor, layer: int, dense: Tensor, to_dense: bool) -> Tensor:
    """One layer's slice of the ray-major network outputs raw (n,l,ns,4) <-> dense (n,ns,4) (stnerf_copy_layer_raw): ``to_dense``
    copies ``raw[:, layer]`` into ``dense``, otherwise ``dense`` into ``raw[:, layer]`` (the other layers stay as they are).
    Returns the tensor written."""
    if raw.dim() != 4 or raw.shape[3] != 4 or tuple(dense.shape) != (raw.shape[0], raw.shape[2], 4):
        raise ValueError(f"copy_layer_raw: raw must be (n,l,ns,4) and dense (n,ns,4), got {tuple(raw.shape)} and {tuple(dense.shape)}")
    n, l, ns = raw.shape[0], raw.shape[1], raw.shape[2]
    hip.check(hip.lib().stnerf_copy_layer_raw(hip.dptr(raw, name="raw"), n, l, int(layer), ns, hip.dptr(dense, name="dense"),
                                              int(bool(to_dense)), hip.stream_ptr()), "stnerf_copy_layer_raw")
    return dense if to_dense else raw


# ---------------------------------------------------------------------------------------- occupancy grids
def copy_layer_raw_listed(raw: Tensor, layer: int, dense: Tensor, rays: Tensor, count: Tensor, to_dense: bool,
                          ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None, mismatch: Optional[Tensor] = None) -> Tensor:
    """The compact sibling of ``copy_layer_raw`` (stnerf_copy_layer_raw_listed; include/stnerf.h states the rule): slot j of dense
    (capacity,ns,4) <-> raw (n,l,ns,4)[rays[j], layer], for a performer ``layer`` >= 1.  ``to_dense`` (capture): ``ray_list`` (int32,
    at least *ray_count entries) and ``ray_count`` (int32, one element) are the frame's list of the layer; ``rays`` (capacity,) int32 and
    ``count`` (one int32) receive the list and its length, or count = -1 and nothing else when it exceeds the capacity.  Otherwise
    (restore) ``rays`` / ``count`` are read and raw[rays[j], layer] = dense[j] for j < count; ``mismatch`` (one int64) += 1 when
    ``ray_count`` is given and differs from count.  Returns the destination.  No host sync: the counts are read on the device."""
    if raw.dim() != 4 or raw.shape[3] != 4 or dense.dim() != 3 or tuple(dense.shape[1:]) != (raw.shape[2], 4):
        raise ValueError(f"copy_layer_raw_listed: raw must be (n,l,ns,4) and dense (capacity,ns,4), got {tuple(raw.shape)} and {tuple(dense.shape)}")
    n, l, ns, capacity = raw.shape[0], raw.shape[1], raw.shape[2], dense.shape[0]
    if rays.numel() < capacity or count.numel() < 1:
        raise ValueError(f"copy_layer_raw_listed: rays must hold {capacity} entries and count one, got {rays.numel()} and {count.numel()}")
    if to_dense and (ray_list is None or ray_count is None or ray_list.numel() < min(n, capacity)):
        # (the kernel reads ray_list[j] for j < *ray_count only when that count is at most min(n, capacity))
        raise ValueError(f"copy_layer_raw_listed: a capture needs ray_count and a ray_list of at least min(n, capacity) = {min(n, capacity)} entries")
    for name, c in (("ray_count", ray_count), ("mismatch", mismatch)):
        if c is not None and c.numel() < 1:
            raise ValueError(f"copy_layer_raw_listed: {name} is empty")
    # (an empty tensor has no storage and the library refuses null pointers: a capacity of 0 travels with a 16-byte stand-in that
    # is never dereferenced; so does the raw of n = 0 rays)
    spare = torch.empty(4, dtype=torch.float32, device=count.device) if capacity == 0 or n == 0 else None
    as_ptr = lambda t, dtype, name: hip.dptr(t if t.numel() else spare.view(dtype), dtype, name)
    hip.check(hip.lib().stnerf_copy_layer_raw_listed(as_ptr(raw, torch.float32, "raw"), n, l, int(layer), ns,
                                                     None if ray_list is None else as_ptr(ray_list, torch.int32, "ray_list"),
                                                     hip.dptr(ray_count, torch.int32, "ray_count"), as_ptr(dense, torch.float32, "dense"),
                                                     as_ptr(rays, torch.int32, "rays"), hip.dptr(count, torch.int32, "count"), capacity,
                                                     int(bool(to_dense)), hip.dptr(mismatch, torch.int64, "mismatch"), hip.stream_ptr()),
              "stnerf_copy_layer_raw_listed")
    return dense if to_dense else raw


def _layer_cache_table(layer_caches, l, n1, n2, only_coarse):
    """-> hip.LayerCache array of l entries.  layer_caches: per layer None | (raw_coarse (capacity,n1,4), raw_fine (capacity,n1+n2,4) |
    None, rays (capacity,) int32, count (1,) int32, mode)."""
    if len(layer_caches) != l:
        raise ValueError(f"layer_caches must have one entry per layer ({l}), got {len(layer_caches)}")
    arr = (hip.LayerCache * l)()
    for i, e in enumerate(layer_caches):
        if e is None:
            continue
        raw_c, raw_f, rays, count, mode = e
        cap = raw_c.shape[0]
        if tuple(raw_c.shape) != (cap, n1, 4) or (raw_f is not None and tuple(raw_f.shape) != (cap, n1 + n2, 4)) or rays.numel() < cap \
                or count.numel() < 1 or (raw_f is None and not only_coarse):
            raise ValueError(f"render_rays: layer cache entry {i} of capacity {cap} must be ({cap},{n1},4), ({cap},{n1 + n2},4), {cap} rays and one count")
        arr[i] = hip.LayerCache(hip.dptr(raw_c, name="layer cache raw_coarse").value, hip.dptr(raw_f, name="layer cache raw_fine").value,
                                hip.dptr(rays, torch.int32, "layer cache rays").value, hip.dptr(count, torch.int32, "layer cache count").value,
                                cap, int(mode))
    return arr


def occupancy_words(res) -> int:
    """uint32 words of a bit table of res = (Rx, Ry, Rz) cells."""
    return (int(res[0]) * int(res[1]) * int(res[2]) + 31) // 32


def occupancy_build(sigma_c: Optional[Tensor], sigma_f: Optional[Tensor], threshold: float, dilate: int) -> Tensor:
    """Vertex densities (Rz+1, Ry+1, Rx+1) of the coarse and / or the fine SpaceNet -> the bit table of the (Rx, Ry, Rz) grid
    (stnerf_occupancy_build; include/stnerf.h states the rule): int32 words holding the uint32 bits, cell c = (z Ry + y) Rx + x
    at bit c & 31 of word c >> 5."""
    given = [s for s in (sigma_c, sigma_f) if s is not None]
    if not given:
        raise ValueError("occupancy_build: one of sigma_c / sigma_f is required")
    if any(s.dim() != 3 or s.shape != given[0].shape for s in given):
        raise ValueError(f"occupancy_build: sigma arrays must be (Rz+1, Ry+1, Rx+1) and alike, got {[tuple(s.shape) for s in given]}")
    res = (given[0].shape[2] - 1, given[0].shape[1] - 1, given[0].shape[0] - 1)
    if min(res) < 1:
        raise ValueError(f"occupancy_build: sigma arrays of shape {tuple(given[0].shape)} hold no cell")
    bits = torch.empty(occupancy_words(res), dtype=torch.int32, device=given[0].device)
    hip.check(hip.lib().stnerf_occupancy_build(hip.dptr(sigma_c, name="sigma_c"), hip.dptr(sigma_f, name="sigma_f"), (C.c_int32 * 3)(*res),
                                               float(threshold), int(dilate), hip.dptr(bits, torch.int32), hip.stream_ptr()),
              "stnerf_occupancy_build")
    return bits


def _occupancy_table(table, l):
    """-> hip.Occupancy array of l entries | None.  table: per layer None | (bits int32 device tensor, (Rx, Ry, Rz), lo (3 floats),
    inv_cell (3 floats)) -- the numbers as they are (``stnerf_amd.occupancy`` computes inv_cell in fp32)."""
    if table is None:
        return None
    if len(table) != l:
        raise ValueError(f"occupancy table must have one entry per layer ({l}), got {len(table)}")
    arr = (hip.Occupancy * l)()
    for i, e in enumerate(table):
        if e is None:
            continue
        bits, res, lo, inv = e
        if min(res) >= 1 and bits.numel() < occupancy_words(res):
            raise ValueError(f"occupancy grid of layer {i}: {bits.numel()} words for res {tuple(res)}, need {occupancy_words(res)}")
        arr[i].bits = hip.dptr(bits, torch.int32, "occupancy bits").value
        for a in range(3):
            arr[i].res[a], arr[i].lo[a], arr[i].inv_cell[a] = int(res[a]), float(lo[a]), float(inv[a])
    return arr


def occupancy_cull(xyz: Tensor, mask: Tensor, table, counts: Optional[Tensor] = None) -> Tensor:
    """Clear bit 0 of mask (n,l) uint8, in place, for every (ray, layer) pair of a layer with a grid none of whose points
    xyz (n,l,n1,3) lies in an occupied cell (stnerf_occupancy_cull).  table: per layer None | (bits, res, lo, inv_cell);
    counts: int32 (l,2) device tensor that accumulates (pairs tested, pairs culled), or None."""
    n, l, n1 = xyz.shape[0], xyz.shape[1], xyz.shape[2]
    if tuple(mask.shape) != (n, l) or xyz.dim() != 4 or xyz.shape[3] != 3:
        raise ValueError(f"occupancy_cull: xyz must be (n,l,n1,3) and mask (n,l), got {tuple(xyz.shape)} and {tuple(mask.shape)}")
    if counts is not None and tuple(counts.shape) != (l, 2):
        raise ValueError(f"occupancy_cull: counts must be ({l},2) int32, got {tuple(counts.shape)}")
    hip.check(hip.lib().stnerf_occupancy_cull(hip.dptr(xyz, name="xyz"), n, l, n1, _occupancy_table(table, l), hip.dptr(mask, torch.uint8, "mask"),
                                              hip.dptr(counts, torch.int32, "counts"), hip.stream_ptr()), "stnerf_occupancy_cull")
    return mask


def _rows_args(what: str, raw: Tensor, xyz: Optional[Tensor], t: Optional[Tensor], t_stop: Optional[Tensor], row_list: Optional[Tensor],
               row_count: Optional[Tensor], counts: Optional[Tensor], layer: Optional[int] = None) -> dict:
    """What the four rows calls share: the shape checks of the layer's slices xyz (n,ns,3), raw (n,ns,4), t (n,ns), of t_stop (n,)
    and of counts -- (2,), or with ``layer`` (> layer, 2) --, the pointer and ray stride of each strided view (an absent xyz or t
    is a null pointer), and the default ``row_list`` (n x ns words) and ``row_count``.  -> the C arguments by name: "xyz" / "t" /
    "raw" = (pointer, ray stride), "rows" = (row_list, capacity, row_count, counts), and "out" = (row_list, row_count)."""
    if xyz is not None and (xyz.dim() != 3 or xyz.shape[2] != 3 or raw.dim() != 3 or tuple(raw.shape) != (xyz.shape[0], xyz.shape[1], 4)):
        raise ValueError(f"{what}: xyz must be (n,ns,3) and raw (n,ns,4), got {tuple(xyz.shape)} and {tuple(raw.shape)}")
    n, ns = raw.shape[0], raw.shape[1]
    if t is not None and tuple(t.shape) != (n, ns):
        raise ValueError(f"{what}: t must be ({n},{ns}), got {tuple(t.shape)}")
    if t_stop is not None and tuple(t_stop.shape) != (n,):
        raise ValueError(f"{what}: t_stop must be ({n},), got {tuple(t_stop.shape)}")
    null = (C.c_void_p(0), 0)
    a = {"n": n, "ns": ns, "xyz": _strided_view_ptr(xyz, (ns, 3), "xyz") if xyz is not None else null,
         "raw": _strided_view_ptr(raw, (ns, 4), "raw"), "t": _strided_view_ptr(t, (ns,), "t") if t is not None else null,
         "t_stop": hip.dptr(t_stop, name="t_stop")}
    if row_list is None:
        row_list = torch.empty(max(n * ns, 1), dtype=torch.int32, device=raw.device)
    if row_count is None:
        row_count = torch.zeros(1, dtype=torch.int32, device=raw.device)
    if counts is not None and layer is None and tuple(counts.shape) != (2,):
        raise ValueError(f"{what}: counts must be int64 (2,), got {tuple(counts.shape)}")
    if counts is not None and layer is not None and (counts.dim() != 2 or counts.shape[1] != 2 or counts.shape[0] <= int(layer)):
        raise ValueError(f"{what}: counts must be int64 (> {int(layer)}, 2), got {tuple(counts.shape)}")
    a["out"] = (row_list, row_count)
    a["rows"] = (hip.dptr(row_list, torch.int32, "row_list"), row_list.numel(), hip.dptr(row_count, torch.int32, "row_count"),
                 hip.dptr(counts, torch.int64, "counts"))
    return a


def occupancy_rows(xyz: Tensor, raw: Tensor, grid, layer: int = 1, ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None,
                   row_list: Optional[Tensor] = None, row_count: Optional[Tensor] = None, counts: Optional[Tensor] = None):
    """One layer's row list of the sample cull (stnerf_occupancy_rows; include/stnerf.h states the rule).  xyz (n,ns,3) and raw
    (n,ns,4) are the layer's slices (strided views whose dim 0 is the ray); grid = (bits, res, lo, inv_cell), the layer's table
    entry; ray_list / ray_count: its work list or None (every ray).  Writes one int32 word ``ray << 8 | k`` per listed sample of
    the listed rays into ``row_list`` (at least n x ns words; made here when None), their number into ``row_count`` (1,), and four
    zero words into raw at every sample of those rays that is NOT listed.  counts: int64 (>= layer + 1, 2) | None accumulates
    (samples tested, samples skipped) in row ``layer``.  -> (row_list, row_count)."""
    if grid is None:
        raise ValueError("occupancy_rows: the layer's grid (bits, res, lo, inv_cell) is required")
    a = _rows_args("occupancy_rows", raw, xyz, None, None, row_list, row_count, counts, layer)
    lp, cp = _worklist(ray_list, ray_count)
    hip.check(hip.lib().stnerf_occupancy_rows(lp, cp, a["n"], int(layer), *a["xyz"], a["ns"], _occupancy_table([grid], 1), *a["raw"], *a["rows"],
                                              hip.stream_ptr()), "stnerf_occupancy_rows")
    return a["out"]


def background_rows(xyz: Tensor, raw: Tensor, grid, t: Optional[Tensor] = None, t_stop: Optional[Tensor] = None,
                    row_list: Optional[Tensor] = None, row_count: Optional[Tensor] = None, counts: Optional[Tensor] = None):
    """Layer 0's row list of one stage under the background's grid (stnerf_background_rows; include/stnerf.h states the rule).
    xyz (n,ns,3) and raw (n,ns,4) are layer 0's slices (strided views whose dim 0 is the ray); grid = (bits, res, lo, inv_cell),
    mandatory.  EVERY ray 0..n-1 is tested: sample k is listed when its point lies in an occupied cell (or has a NaN coordinate)
    and -- with t (n,ns) and t_stop (n,), ``ray_stop``'s output -- ``not t[ray, k] > t_stop[ray]``; the others get four zero words
    in raw.  counts: int64 (2,) | None accumulates (samples tested, not listed).  -> (row_list, row_count)."""
    if grid is None:
        raise ValueError("background_rows: the background's grid (bits, res, lo, inv_cell) is required")
    a = _rows_args("background_rows", raw, xyz, t, t_stop, row_list, row_count, counts)
    hip.check(hip.lib().stnerf_background_rows(a["n"], *a["xyz"], a["ns"], _occupancy_table([grid], 1), *a["t"], a["t_stop"], *a["raw"], *a["rows"],
                                               hip.stream_ptr()), "stnerf_background_rows")
    return a["out"]


def background_ray_rows(xyz: Tensor, raw: Tensor, ray_flags: Tensor, grid=None, t: Optional[Tensor] = None, t_stop: Optional[Tensor] = None,
                        row_list: Optional[Tensor] = None, row_count: Optional[Tensor] = None, counts: Optional[Tensor] = None):
    """Layer 0's row list of one stage under a per-ray mask (stnerf_background_ray_rows; include/stnerf.h states the rule):
    ``background_rows`` with ``ray_flags`` (n,) uint8 or bool in front of its tests and the grid optional.  Sample k of ray r is
    listed when ``ray_flags[r]`` is nonzero and -- with ``grid`` = (bits, res, lo, inv_cell) -- its point lies in an occupied cell (or
    has a NaN coordinate) and -- with t (n,ns) and t_stop (n,) -- ``not t[r, k] > t_stop[r]``; the others get four zero words in
    raw.  A ray whose flag is zero lists nothing and loads nothing.  counts: int64 (2,) | None accumulates (samples tested, not
    listed).  -> (row_list, row_count)."""
    a = _rows_args("background_ray_rows", raw, xyz, t, t_stop, row_list, row_count, counts)
    flags = _ray_flags(ray_flags, a["n"], "background_ray_rows")
    entry = None if grid is None else _occupancy_table([grid], 1)
    hip.check(hip.lib().stnerf_background_ray_rows(a["n"], *a["xyz"], a["ns"], entry, *a["t"], a["t_stop"], *a["raw"], *a["rows"],
                                                   hip.dptr(flags, torch.uint8, "ray_flags"), hip.stream_ptr()), "stnerf_background_ray_rows")
    return a["out"]


def _density_grid_table(table, l):
    """-> hip.DensityGrid array of l entries | None.  table: per layer None | (sigma fp32 device tensor (Rz+1, Ry+1, Rx+1), lo (3 floats),
    inv_cell (3 floats)) -- the numbers as they are (``stnerf_amd.proposal`` computes inv_cell in fp32).  A table without a grid is None."""
    if table is None:
        return None
    if len(table) != l:
        raise ValueError(f"proposal table must have one entry per layer ({l}), got {len(table)}")
    if all(e is None for e in table):
        return None
    arr = (hip.DensityGrid * l)()
    for i, e in enumerate(table):
        if e is None:
            continue
        sigma, lo, inv = e
        if not torch.is_tensor(sigma) or sigma.dim() != 3 or min(sigma.shape) < 2:
            raise ValueError(f"density grid of layer {i}: sigma must be a (Rz+1, Ry+1, Rx+1) tensor with a cell per axis, got "
                             f"{tuple(sigma.shape) if torch.is_tensor(sigma) else type(sigma).__name__}")
        arr[i].sigma = hip.dptr(sigma, name=f"density grid of layer {i}").value
        for a in range(3):
            arr[i].res[a], arr[i].lo[a], arr[i].inv_cell[a] = int(sigma.shape[2 - a]) - 1, float(lo[a]), float(inv[a])
    return arr


def proposal_density(xyz: Tensor, raw: Tensor, grid, layer: int = 1, ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None) -> Tensor:
    """One layer's coarse densities from its density grid (stnerf_proposal_density; include/stnerf.h states the rule).  xyz (n,ns,3)
    and raw (n,ns,4) are the layer's slices (strided views whose dim 0 is the ray); grid = (sigma (Rz+1, Ry+1, Rx+1), lo, inv_cell);
    ray_list / ray_count: its work list, or None = every ray.  Every sample of a listed ray gets raw = (0, 0, 0, sigma), the trilinear
    lookup at its point; the rows of the other rays keep their bytes.  -> raw."""
    if grid is None:
        raise ValueError("proposal_density: the layer's grid (sigma, lo, inv_cell) is required")
    if xyz.dim() != 3 or xyz.shape[2] != 3 or raw.dim() != 3 or tuple(raw.shape) != (xyz.shape[0], xyz.shape[1], 4):
        raise ValueError(f"proposal_density: xyz must be (n,ns,3) and raw (n,ns,4), got {tuple(xyz.shape)} and {tuple(raw.shape)}")
    n, ns = raw.shape[0], raw.shape[1]
    if (ray_list is None) != (ray_count is None):
        raise ValueError("proposal_density: ray_list and ray_count come together (both None: every ray)")
    if ray_list is not None and (ray_list.numel() < n or ray_count.numel() < 1):
        raise ValueError(f"proposal_density: ray_list must hold {n} entries and ray_count one, got {ray_list.numel()} and {ray_count.numel()}")
    if n == 0:
        return raw
    lp, cp = _worklist(ray_list, ray_count)
    hip.check(hip.lib().stnerf_proposal_density(lp, cp, n, int(layer), *_strided_view_ptr(xyz, (ns, 3), "xyz"), ns, _density_grid_table([grid], 1),
                                                *_strided_view_ptr(raw, (ns, 4), "raw"), hip.stream_ptr()), "stnerf_proposal_density")
    return raw


def _ray_flags(flags: Tensor, n: int, what: str) -> Tensor:
    """A per-ray mask as the library takes it: (n,) uint8, contiguous, on the device (bool is reinterpreted, not copied)."""
    if not torch.is_tensor(flags) or tuple(flags.shape) != (n,) or flags.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{what}: the per-ray background mask must be a ({n},) uint8 or bool tensor, got "
                         f"{(tuple(flags.shape), flags.dtype) if torch.is_tensor(flags) else type(flags).__name__}")
    flags = flags.contiguous()
    return flags.view(torch.uint8) if flags.dtype == torch.bool else flags


def ray_stop(t: Tensor, merged_weights: Tensor, tau: float) -> Tensor:
    """The stop depth of early ray termination (stnerf_ray_stop; include/stnerf.h states the rule): t (n,l,n1) coarse depths and
    merged_weights (n,l,n1), ``composite_scene``'s coarse merged weights, -> t_stop (n,): the depth of the merged sample after the
    first one at which 1 - (running sum of the merged weights) is no longer above ``tau``; +inf where the ray never gets there."""
    if t.dim() != 3 or tuple(merged_weights.shape) != tuple(t.shape):
        raise ValueError(f"ray_stop: t and merged_weights must be (n,l,n1) alike, got {tuple(t.shape)} and {tuple(merged_weights.shape)}")
    n, l, n1 = t.shape
    out = torch.empty(n, dtype=torch.float32, device=t.device)
    hip.check(hip.lib().stnerf_ray_stop(hip.dptr(t, name="t"), hip.dptr(merged_weights, name="merged_weights"), n, l, n1, float(tau),
                                        hip.dptr(out), hip.stream_ptr()), "stnerf_ray_stop")
    return out


def visibility_rows(t: Tensor, t_stop: Tensor, raw: Tensor, xyz: Optional[Tensor] = None, grid=None, layer: int = 1,
                    ray_list: Optional[Tensor] = None, ray_count: Optional[Tensor] = None, row_list: Optional[Tensor] = None,
                    row_count: Optional[Tensor] = None, counts: Optional[Tensor] = None):
    """One layer's fine row list under early ray termination (stnerf_visibility_rows): ``occupancy_rows`` with the hidden-sample
    test.  t (n,ns) and raw (n,ns,4) are the layer's slices (strided views whose dim 0 is the ray), t_stop (n,) ``ray_stop``'s
    output.  Sample k of a listed ray is listed when ``not t[ray, k] > t_stop[ray]`` and -- with ``grid`` = (bits, res, lo,
    inv_cell) and the layer's points xyz (n,ns,3) -- its point lies in an occupied cell; the others get four zero words in raw.
    ``layer`` 0 is allowed (without a grid).  counts: int64 (>= layer + 1, 2) | None.  -> (row_list, row_count)."""
    if t.dim() != 2 or raw.dim() != 3 or tuple(raw.shape) != (t.shape[0], t.shape[1], 4) or tuple(t_stop.shape) != (t.shape[0],):
        raise ValueError(f"visibility_rows: t must be (n,ns), raw (n,ns,4) and t_stop (n,), got {tuple(t.shape)}, {tuple(raw.shape)}, {tuple(t_stop.shape)}")
    n, ns = t.shape
    if grid is not None and (xyz is None or tuple(xyz.shape) != (n, ns, 3)):
        raise ValueError(f"visibility_rows: a grid needs the layer's points xyz ({n},{ns},3)")
    a = _rows_args("visibility_rows", raw, xyz if grid is not None else None, t, t_stop, row_list, row_count, counts, layer)
    entry = None if grid is None else _occupancy_table([grid], 1)
    lp, cp = _worklist(ray_list, ray_count)
    hip.check(hip.lib().stnerf_visibility_rows(lp, cp, n, int(layer), *a["xyz"], *a["t"], a["t_stop"], ns, entry, *a["raw"], *a["rows"],
                                               hip.stream_ptr()), "stnerf_visibility_rows")
    return a["out"]


def render_rays(rays: Tensor, boxes: Tensor, nets: "hip.Nets", params: "hip.RenderParams", workspace: Tensor,
                jitter: Optional[Tensor] = None, u: Optional[Tensor] = None, cache=None, rotations=None, scene: bool = False,
                layer_alpha: Optional[Sequence[float]] = None, occupancy=None, occupancy_counts: Optional[Tensor] = None,
                occupancy_samples=None, sample_counts: Optional[Tensor] = None, terminate=None, tau: float = 1e-4,
                visibility_counts: Optional[Tensor] = None, background_grid=None, background_counts: Optional[Tensor] = None,
                layer_caches=None, layer_mismatch: Optional[Tensor] = None, occluder: Optional[Tensor] = None,
                occluder_stops: bool = False, background_rays: Optional[Tensor] = None, deep: Optional[dict] = None, proposal=None):
    """One call = the whole chunk pipeline (stnerf_render_rays).  Returns mixed_fine (n,5), mixed_coarse (n,5),
    layer_fine (n,l,5), layer_coarse (n,l,5), mask (n,l) uint8 (fine outputs alias the coarse ones if only_coarse).
    ``cache`` = (raw_coarse (n,n1,4), raw_fine (n,n1+n2,4) | None, mode): the background cache of this launch piece
    (stnerf_render_rays_cached; mode hip.BKGD_CACHE_CAPTURE fills the two tensors, hip.BKGD_CACHE_REUSE renders from them).
    ``rotations``: per layer None | (m, centre), the pairs of ``LayeredRFRender.layer_ray_transforms`` (stnerf_render_rays_rot).
    ``scene``: append the in-scene layer passes of the final stage, (n,l,5) (stnerf_render_rays_scene), to the returned tuple.
    ``layer_alpha``: params.l density factors, one per layer, for the fine composite (stnerf_render_rays_opacity; the library
    refuses an entry that is negative or not finite); params.alpha is ignored then.  None: params.alpha on layer 2, as ever.
    ``occupancy``: per layer None | (bits, res, lo, inv_cell), the table of ``occupancy_cull`` (stnerf_render_rays_occupancy): performer
    pairs whose coarse points all lie in empty cells are dropped before the networks; ``occupancy_counts``: int32 (l,2) | None.
    ``occupancy_samples``: per layer a flag, or None -- a flagged layer (it needs a grid) is sample-culled too: both stages evaluate
    only the samples whose point lies in an occupied cell, the others get zero outputs (stnerf_render_rays_samples; the workspace is
    ``render_workspace_bytes(..., occupancy_samples=...)``); ``sample_counts``: int64 (l,2) | None = (samples tested, skipped).
    ``terminate``: per layer a flag, or None -- early ray termination of the flagged layers' FINE stage (stnerf_render_rays_terminated;
    include/stnerf.h states the rule): fine samples behind the depth at which the coarse pass leaves a transmittance of at most
    ``tau`` get zero outputs and no network evaluation.  Layer 0 may be flagged.  The workspace is
    ``render_workspace_bytes(..., terminate=...)``; ``visibility_counts``: int64 (l,2) | None = (fine samples tested, not listed).
    The library refuses (ValueError, before any launch) tau outside [0, 1), alpha != 1, a layer_alpha entry != 1, precision 2.
    ``background_grid``: None | (bits, res, lo, inv_cell), the background's own grid (stnerf_render_rays_background; include/stnerf.h
    states the rule): in every stage layer 0 is evaluated in, only its samples in occupied cells reach the networks, the others get
    zero outputs.  The workspace is ``render_workspace_bytes(..., background=True)``; ``background_counts``: int64 (2,) | None =
    (samples tested, not listed).  The library refuses precision 2.  An entry whose bits are None is no grid: the call makes
    stnerf_render_rays_terminated's launches.
    ``layer_caches``: per layer None | (raw_coarse (capacity,n1,4), raw_fine (capacity,n1+n2,4) | None, rays (capacity,) int32, count (1,)
    int32, mode), the layer cache's table (stnerf_render_rays_layers; include/stnerf.h states the rules): hip.LAYER_CACHE_CAPTURE fills
    the entry from the layer's hit rays, hip.LAYER_CACHE_REUSE leaves the layer out of the network stages and copies the slices in.
    Entry 0 must be None.  ``layer_mismatch``: int64 (1,) | None, += 1 per restore whose frame has another hit count than the entry.
    ``occluder``: (n,5) rows {r, g, b, a, z} | None, a depth-tested occluder composited into the final stage (stnerf_render_rays_occluded;
    include/stnerf.h states the rules; z in ray-parameter units, ``ray_parameter``).  It needs ``scene=True`` and appends
    occluded_mixed (n,5), occluded_scene (n,l,5) and occluder_share (n,5) to the returned tuple.  ``occluder_stops``: an opaque row
    also lowers the stop depth of early ray termination (needs a ``terminate`` flag); the three occluded outputs keep their bits.
    ``background_rays``: (n,) uint8 or bool | None, the per-ray background mask (stnerf_render_options.bkgd_rays; include/stnerf.h
    states the rule): layer 0 is evaluated only on the rays whose entry is nonzero, the others get zero outputs for it in both
    stages.  It composes with ``background_grid`` and with termination of layer 0 in the one rows launch layer 0 gets per stage.  The
    workspace is ``render_workspace_bytes(..., background_rays=True)``.  The library refuses precision 2 and a background cache in
    CAPTURE or REUSE.
    ``deep``: None | dict(w_min=0.0, merge_dz=0.0, capacity=None), deep output of the final stage (stnerf_render_options_deep;
    include/stnerf.h states the rules).  It needs ``scene=True`` and appends offsets (n+1,) int64, samples (capacity,8) and total (1,)
    int64 to the returned tuple; capacity None = the worst case n l S.  Rays whose records would pass the capacity are not written:
    compare total with the capacity.  The render workspace is the same with or without it.
    ``proposal``: per layer None | (sigma (Rz+1, Ry+1, Rx+1), lo, inv_cell), the table of grid proposals
    (stnerf_render_options_proposal; include/stnerf.h states the rules): a layer with an entry is in no coarse network stage, its coarse
    densities are ``proposal_density``'s.  Its layer_coarse / mixed_coarse carry zero colour and the grid's depth and alpha.  The render
    workspace is the same with or without it.  The library refuses precision 2, a hidden or cached flagged layer, and layer 0 flagged
    beside a background cache, grid or per-ray mask."""
    n, l = rays.shape[0], params.l
    proposal = _density_grid_table(proposal, l)
    if deep is not None:
        if not scene:
            raise ValueError("render_rays: deep output needs scene=True (the merged weights exist only with the scene passes)")
        if set(deep) - {"w_min", "merge_dz", "capacity"}:
            raise ValueError(f"render_rays: deep takes w_min, merge_dz and capacity, got {sorted(deep)}")
    if occluder is not None:
        if not scene:
            raise ValueError("render_rays: an occluder needs scene=True (the merged weights exist only with the scene passes)")
        if tuple(occluder.shape) != (n, 5):
            raise ValueError(f"render_rays: the occluder of {n} rays must be ({n},5) rows of (r, g, b, a, z), got {tuple(occluder.shape)}")
    elif occluder_stops:
        raise ValueError("render_rays: occluder_stops without an occluder")
    bp, bstride, lb = _boxes_arg(boxes, n)
    if lb != l:
        raise ValueError(f"boxes carry {lb} layers, params.l = {l}")
    dev = rays.device
    mix_c = torch.empty(n, 5, dtype=torch.float32, device=dev)
    lo_c = torch.empty(n, l, 5, dtype=torch.float32, device=dev)
    mask = torch.empty(n, l, dtype=torch.uint8, device=dev)
    if params.only_coarse:
        mix_f, lo_f = None, None
    else:
        mix_f = torch.empty(n, 5, dtype=torch.float32, device=dev)
        lo_f = torch.empty(n, l, 5, dtype=torch.float32, device=dev)
    # every optional argument, checked once and named once (stnerf_render_options); what is given but inert -- tau without a flag, count
    # tensors without their feature -- travels as it is: the library ignores it
    record = hip.RenderOptionsProposal if proposal is not None else hip.RenderOptions if deep is None else hip.RenderOptionsDeep
    opts = record(tau=float(tau), occluder_stops=int(bool(occluder_stops)))
    if proposal is not None:
        opts.proposal = proposal
    opts.rot = _rotations(rotations, l)
    if cache is not None:
        raw_c, raw_f, mode = cache
        S = params.n1 + params.n2
        if tuple(raw_c.shape) != (n, params.n1, 4) or (raw_f is not None and tuple(raw_f.shape) != (n, S, 4)):
            raise ValueError(f"render_rays: the background cache of {n} rays must be ({n},{params.n1},4) and ({n},{S},4)")
        opts.cache = C.pointer(hip.BkgdCache(hip.dptr(raw_c, name="cache raw_coarse").value, hip.dptr(raw_f, name="cache raw_fine").value, int(mode)))
    scene_out = torch.empty(n, l, 5, dtype=torch.float32, device=dev) if scene else None
    opts.scene_out = hip.dptr(scene_out)
    if layer_alpha is not None:
        if len(layer_alpha) != l:
            raise ValueError(f"layer_alpha must have one entry per layer ({l}), got {len(layer_alpha)}")
        opts.layer_alpha = (C.c_float * l)(*(float(a) for a in layer_alpha))
    opts.occ = _occupancy_table(occupancy, l)
    if occupancy_samples is not None and any(occupancy_samples):
        if occupancy is None or len(occupancy_samples) != l:
            raise ValueError(f"occupancy_samples needs an occupancy table and one flag per layer ({l})")
        opts.samples = _layer_flags(occupancy_samples, l, "occupancy_samples")
    if terminate is not None:
        opts.terminate = _layer_flags(terminate, l, "terminate")
    for name, c in (("occupancy_counts", occupancy_counts), ("sample_counts", sample_counts), ("visibility_counts", visibility_counts)):
        if c is not None and tuple(c.shape) != (l, 2):
            raise ValueError(f"{name} must be ({l},2), got {tuple(c.shape)}")
    if background_counts is not None and tuple(background_counts.shape) != (2,):
        raise ValueError(f"background_counts must be int64 (2,), got {tuple(background_counts.shape)}")
    if layer_mismatch is not None and layer_mismatch.numel() < 1:
        raise ValueError("layer_mismatch must hold one int64")
    opts.counts = hip.dptr(occupancy_counts, torch.int32, "occupancy_counts")
    opts.sample_counts = hip.dptr(sample_counts, torch.int64, "sample_counts")
    opts.visibility_counts = hip.dptr(visibility_counts, torch.int64, "visibility_counts")
    opts.bkgd_counts = hip.dptr(background_counts, torch.int64, "background_counts")
    opts.mismatch = hip.dptr(layer_mismatch, torch.int64, "layer_mismatch")
    if background_grid is not None:   # (an entry whose bits are None is no grid)
        opts.bkgd_grid = (hip.Occupancy * 1)() if background_grid[0] is None else _occupancy_table([background_grid], 1)
    if background_rays is not None:
        background_rays = _ray_flags(background_rays, n, "render_rays")
        opts.bkgd_rays = hip.dptr(background_rays, torch.uint8, "background_rays")
    if layer_caches is not None:
        opts.layers = _layer_cache_table(layer_caches, l, params.n1, params.n2, bool(params.only_coarse))
    occ_out = None
    if occluder is not None:
        occ_out = (torch.empty(n, 5, dtype=torch.float32, device=dev), torch.empty(n, l, 5, dtype=torch.float32, device=dev),
                   torch.empty(n, 5, dtype=torch.float32, device=dev))
        occluder = occluder.contiguous()
        opts.occluder = hip.dptr(occluder, name="occluder")
        opts.occluded_mixed, opts.occluded_scene, opts.occluder_share = (hip.dptr(t) for t in occ_out)
    deep_out = None
    if deep is not None:
        S_final = params.n1 if params.only_coarse else params.n1 + params.n2
        capacity = deep.get("capacity")
        capacity = n * l * S_final if capacity is None else int(capacity)
        if capacity < 0:
            raise ValueError(f"render_rays: deep capacity = {capacity}")
        scan = deep_workspace_bytes(n)
        deep_out = (torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(max(capacity, 1), 8, dtype=torch.float32, device=dev)[:capacity],
                    torch.zeros(1, dtype=torch.int64, device=dev))
        deep_ws = torch.empty((scan + 4 * n + 7) // 8 + 1, dtype=torch.int64, device=dev)
        opts.deep_w_min, opts.deep_merge_dz, opts.deep_capacity = float(deep.get("w_min", 0.0)), float(deep.get("merge_dz", 0.0)), capacity
        opts.deep_offsets, opts.deep_total = hip.dptr(deep_out[0], torch.int64), hip.dptr(deep_out[2], torch.int64)
        opts.deep_samples, opts.deep_workspace = C.c_void_p(deep_out[1].data_ptr()), hip.dptr(deep_ws, torch.int64)
    hip.check(hip.lib().stnerf_render_rays_opts(hip.dptr(rays, name="rays"), n, bp, bstride, C.byref(nets), C.byref(params),
                                                hip.dptr(jitter, name="jitter"), hip.dptr(u, name="u"),
                                                hip.dptr(workspace, torch.uint8, "workspace"), workspace.numel(),
                                                hip.dptr(mix_f), hip.dptr(mix_c), hip.dptr(lo_f), hip.dptr(lo_c), hip.dptr(mask, torch.uint8),
                                                C.byref(opts) if record is hip.RenderOptions else opts.ref(), hip.stream_ptr()), "stnerf_render_rays")
    out = (mix_c, mix_c, lo_c, lo_c, mask) if params.only_coarse else (mix_f, mix_c, lo_f, lo_c, mask)
    out = out + (scene_out,) if scene else out
    out = out + occ_out if occ_out is not None else out
    return out + deep_out if deep_out is not None else out


# ---------------------------------------------------------------------------------------- depth-tested occluders
def scene_occluder(t: Tensor, raw: Tensor, mask: Optional[Tensor], merged_weights: Tensor, scene: Tensor, mixed: Tensor,
                   occluder: Tensor, params: Optional["hip.CompositeParams"] = None, rgb_activated: bool = False,
                   evaluated: Optional[Sequence[int]] = None, want_scene: bool = True, want_share: bool = True,
                   want_front_behind: bool = False):
    """A depth-tested occluder on the merged weights of a finished composite (stnerf_scene_occluder; include/stnerf.h states the
    rules).  t (n,l,S), raw (n,l,S,4), mask (n,l) uint8 | None, merged_weights (n,l,S), scene (n,l,5) and mixed (n,5) are what
    ``composite_scene`` took and returned (``params``: its stnerf_composite_params, of which rgb_activated and evaluated are
    read; None: built from the two keywords).  occluder (n,5): rows {r, g, b, a, z}, z in ray-parameter units.  ->
    (occluded_mixed (n,5), occluded_scene (n,l,5) | None, occluder_share (n,5) | None, front (n,l,5) | None, behind (n,l,5) | None):
    the mixed image with the occluder in the scene, every layer's share of it, the occluder's own premultiplied share, and the
    two halves of every layer's scene pass in front of and behind z.  Rows with a <= 0 or a z that is not finite are absent: the
    plain outputs come back."""
    if t.dim() != 3 or tuple(raw.shape) != tuple(t.shape) + (4,) or tuple(merged_weights.shape) != tuple(t.shape):
        raise ValueError(f"scene_occluder: t and merged_weights must be (n,l,S) and raw (n,l,S,4), got {tuple(t.shape)}, "
                         f"{tuple(merged_weights.shape)}, {tuple(raw.shape)}")
    n, l, S = t.shape
    if tuple(scene.shape) != (n, l, 5) or tuple(mixed.shape) != (n, 5) or tuple(occluder.shape) != (n, 5):
        raise ValueError(f"scene_occluder: scene must be ({n},{l},5), mixed and occluder ({n},5), got {tuple(scene.shape)}, "
                         f"{tuple(mixed.shape)}, {tuple(occluder.shape)}")
    p = params if params is not None else composite_params(evaluated=evaluated, rgb_activated=rgb_activated)
    dev = t.device
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    out_mixed = new(n, 5)
    out_scene = new(n, l, 5) if want_scene else None
    share = new(n, 5) if want_share else None
    front = new(n, l, 5) if want_front_behind else None
    behind = new(n, l, 5) if want_front_behind else None
    hip.check(hip.lib().stnerf_scene_occluder(hip.dptr(t, name="t"), hip.dptr(raw, name="raw"), hip.dptr(mask, torch.uint8, "mask"),
                                              hip.dptr(merged_weights, name="merged_weights"), n, l, S, C.byref(p),
                                              hip.dptr(scene, name="scene"), hip.dptr(mixed, name="mixed"),
                                              hip.dptr(occluder, name="occluder"), hip.dptr(out_mixed), hip.dptr(out_scene),
                                              hip.dptr(share), hip.dptr(front), hip.dptr(behind), hip.stream_ptr()),
              "stnerf_scene_occluder")
    return out_mixed, out_scene, share, front, behind


def occluder_stop(occluder: Tensor, t_stop: Tensor) -> Tensor:
    """Fold the opaque rows of an occluder (n,5) into early ray termination's stop depths t_stop (n,), IN PLACE
    (stnerf_occluder_stop): a present row with a >= 1 and z < t_stop[ray] makes z the ray's stop depth.  -> t_stop."""
    if occluder.dim() != 2 or occluder.shape[1] != 5 or tuple(t_stop.shape) != (occluder.shape[0],):
        raise ValueError(f"occluder_stop: occluder must be (n,5) and t_stop (n,), got {tuple(occluder.shape)} and {tuple(t_stop.shape)}")
    hip.check(hip.lib().stnerf_occluder_stop(hip.dptr(occluder, name="occluder"), occluder.shape[0], hip.dptr(t_stop, name="t_stop"),
                                             hip.stream_ptr()), "stnerf_occluder_stop")
    return t_stop


# ---------------------------------------------------------------------------------------- deep frames
def deep_workspace_bytes(n: int) -> int:
    """Bytes of scratch ``deep_offsets`` needs for n rays (stnerf_deep_workspace_bytes); not part of the render workspace."""
    b = hip.lib().stnerf_deep_workspace_bytes(int(n))
    hip.check(b if b < 0 else hip.OK, "stnerf_deep_workspace_bytes")
    return int(b)


def _deep_ray_args(what, t, mask, merged_weights, params, rgb_activated, evaluated):
    if t.dim() != 3 or tuple(merged_weights.shape) != tuple(t.shape):
        raise ValueError(f"{what}: t and merged_weights must be (n,l,S) alike, got {tuple(t.shape)} and {tuple(merged_weights.shape)}")
    if mask is not None and tuple(mask.shape) != tuple(t.shape[:2]):
        raise ValueError(f"{what}: mask must be {tuple(t.shape[:2])}, got {tuple(mask.shape)}")
    return params if params is not None else composite_params(evaluated=evaluated, rgb_activated=rgb_activated)


def deep_count(t: Tensor, mask: Optional[Tensor], merged_weights: Tensor, w_min: float = 0.0, merge_dz: float = 0.0,
               params: Optional["hip.CompositeParams"] = None, rgb_activated: bool = False, evaluated: Optional[Sequence[int]] = None,
               counts: Optional[Tensor] = None) -> Tensor:
    """The deep segments of every ray (stnerf_deep_count; include/stnerf.h states the rules): t, merged_weights (n,l,S) and mask
    (n,l) uint8 | None as ``composite_scene`` took and left them -> counts (n,) int32."""
    p = _deep_ray_args("deep_count", t, mask, merged_weights, params, rgb_activated, evaluated)
    n, l, S = t.shape
    if counts is None:
        counts = torch.empty(n, dtype=torch.int32, device=t.device)
    elif tuple(counts.shape) != (n,):
        raise ValueError(f"deep_count: counts must be ({n},), got {tuple(counts.shape)}")
    hip.check(hip.lib().stnerf_deep_count(hip.dptr(t, name="t"), hip.dptr(mask, torch.uint8, "mask"), hip.dptr(merged_weights, name="merged_weights"),
                                          n, l, S, C.byref(p), float(w_min), float(merge_dz), hip.dptr(counts, torch.int32, "counts"),
                                          hip.stream_ptr()), "stnerf_deep_count")
    return counts


def deep_offsets(counts: Tensor, max_count: int, offsets: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """counts (n,) int32, each at most ``max_count`` (l S) -> offsets (n+1,) int64, their ordered exclusive scan and the total
    (stnerf_deep_offsets).  workspace: uint8, at least ``deep_workspace_bytes(n)``; None: made here."""
    n = counts.shape[0]
    if offsets is None:
        offsets = torch.empty(n + 1, dtype=torch.int64, device=counts.device)
    elif tuple(offsets.shape) != (n + 1,):
        raise ValueError(f"deep_offsets: offsets must be ({n + 1},), got {tuple(offsets.shape)}")
    if workspace is None:
        workspace = torch.empty(deep_workspace_bytes(n), dtype=torch.uint8, device=counts.device)
    hip.check(hip.lib().stnerf_deep_offsets(hip.dptr(counts, torch.int32, "counts"), n, int(max_count), hip.dptr(offsets, torch.int64, "offsets"),
                                            hip.dptr(workspace, torch.uint8, "workspace"), workspace.numel(), hip.stream_ptr()),
              "stnerf_deep_offsets")
    return offsets


def deep_fill(t: Tensor, raw: Tensor, mask: Optional[Tensor], merged_weights: Tensor, offsets: Tensor, samples: Tensor,
              w_min: float = 0.0, merge_dz: float = 0.0, params: Optional["hip.CompositeParams"] = None, rgb_activated: bool = False,
              evaluated: Optional[Sequence[int]] = None, total: Optional[Tensor] = None):
    """The deep records at ``offsets`` (stnerf_deep_fill): raw (n,l,S,4); samples (capacity,8) is written in place, a ray whose range
    would pass the capacity is left unwritten.  -> (samples, total (1,) int64 = the records needed, whatever the capacity)."""
    p = _deep_ray_args("deep_fill", t, mask, merged_weights, params, rgb_activated, evaluated)
    n, l, S = t.shape
    if tuple(raw.shape) != (n, l, S, 4) or tuple(offsets.shape) != (n + 1,) or samples.dim() != 2 or samples.shape[1] != 8:
        raise ValueError(f"deep_fill: raw must be ({n},{l},{S},4), offsets ({n + 1},) and samples (capacity,8), got {tuple(raw.shape)}, "
                         f"{tuple(offsets.shape)}, {tuple(samples.shape)}")
    if total is None:
        total = torch.zeros(1, dtype=torch.int64, device=t.device)
    hip.check(hip.lib().stnerf_deep_fill(hip.dptr(t, name="t"), hip.dptr(raw, name="raw"), hip.dptr(mask, torch.uint8, "mask"),
                                         hip.dptr(merged_weights, name="merged_weights"), n, l, S, C.byref(p), float(w_min), float(merge_dz),
                                         hip.dptr(offsets, torch.int64, "offsets"), hip.dptr(samples, name="samples"), samples.shape[0],
                                         hip.dptr(total, torch.int64, "total"), hip.stream_ptr()), "stnerf_deep_fill")
    return samples, total


def deep_composite(offsets: Tensor, samples: Tensor, l: int, elements: Optional[Tensor] = None, want_scene: bool = True,
                   want_shares: bool = True):
    """Depth-tested elements composited on a deep list (stnerf_deep_composite; include/stnerf.h states the rules): offsets (n+1,)
    int64, samples (total,8), elements (n,E,5) rows {r, g, b, a, z}, 0 <= E <= 8, or None = the flatten.  -> (mixed (n,5), scene
    (n,l,5) | None, shares (n,E,5) | None)."""
    n = offsets.shape[0] - 1
    if offsets.dim() != 1 or n < 0 or samples.dim() != 2 or samples.shape[1] != 8:
        raise ValueError(f"deep_composite: offsets must be (n+1,) and samples (total,8), got {tuple(offsets.shape)} and {tuple(samples.shape)}")
    E = 0 if elements is None else elements.shape[1] if elements.dim() == 3 else -1
    if elements is not None and (E < 0 or tuple(elements.shape) != (n, E, 5)):
        raise ValueError(f"deep_composite: elements must be ({n},E,5) rows of (r, g, b, a, z), got {tuple(elements.shape)}")
    dev = offsets.device
    mixed = torch.empty(n, 5, dtype=torch.float32, device=dev)
    scene = torch.empty(n, int(l), 5, dtype=torch.float32, device=dev) if want_scene else None
    shares = torch.empty(n, E, 5, dtype=torch.float32, device=dev) if want_shares and E > 0 else None
    hip.check(hip.lib().stnerf_deep_composite(hip.dptr(offsets, torch.int64, "offsets"), hip.dptr(samples, name="samples") if samples.numel() else None,
                                              n, int(l), hip.dptr(elements, name="elements") if E > 0 else None, E, hip.dptr(mixed),
                                              hip.dptr(scene), hip.dptr(shares), hip.stream_ptr()), "stnerf_deep_composite")
    return mixed, scene, shares


def ray_parameter(rays: Tensor, pose: Tensor, zcam) -> Tensor:
    """The ray parameter t at which o + t d has camera-space depth ``zcam``: t = zcam / (d . forward), with forward = pose[:3, 2],
    the viewing axis ``generate_rays`` rotates the pixel directions by.  This is how a renderer's z-buffer becomes the z of an
    occluder row.  rays (n, >= 6), pose (4,4) or (3,4) camera-to-world, zcam (n,) or a scalar; plain torch, host or device."""
    d = rays[:, 3:6]
    forward = torch.as_tensor(pose, dtype=d.dtype)[:3, 2].to(d.device)
    z = torch.as_tensor(zcam, dtype=d.dtype).to(d.device)
    return z / (d * forward).sum(-1)


# ---------------------------------------------------------------------------------------- progressive multi-sample frames
class AccumulateState:
    """Per-pixel running statistics of a progressive frame (include/stnerf.h: stnerf_accumulate): ``mean`` (P,C), ``m2`` (P,V)
    -- the second moment of the first V columns -- and ``count`` (P,) int32, all zero at first; plus the buffers
    ``accumulate_select`` writes (made on first use)."""

    def __init__(self, n_pixels: int, C_: int, V: int = 3, device="cuda"):
        if n_pixels < 1 or not (1 <= V <= C_):
            raise ValueError(f"accumulate_state: need n_pixels >= 1 and 1 <= V <= C, got n_pixels={n_pixels}, C={C_}, V={V}")
        self.mean = torch.zeros(n_pixels, C_, dtype=torch.float32, device=device)
        self.m2 = torch.zeros(n_pixels, V, dtype=torch.float32, device=device)
        self.count = torch.zeros(n_pixels, dtype=torch.int32, device=device)
        self._select = None

    @property
    def n_pixels(self) -> int:
        return self.count.shape[0]


def accumulate_state(n_pixels: int, C_: int, V: int = 3, device="cuda") -> AccumulateState:
    """A zeroed ``AccumulateState`` for n_pixels pixels of C floats, the first V with a second moment."""
    return AccumulateState(n_pixels, C_, V, device)


def accumulate(values: Tensor, state: AccumulateState, pixels: Optional[Tensor] = None) -> AccumulateState:
    """One more sample of some pixels, IN PLACE (stnerf_accumulate: Welford's update, every fp32 operation on its own).
    values (n,C): a 2-D float32 device view with dense columns (any row stride); row i belongs to pixel ``pixels[i]`` -- a device
    int32 list that names a pixel at most once -- or to pixel i without a list.  A pixel's first sample becomes its mean as it
    is.  -> state."""
    vp, stride = _mat(values, "values")
    n, C_ = values.shape
    if C_ != state.mean.shape[1]:
        raise ValueError(f"accumulate: values are {C_} floats wide, the state {state.mean.shape[1]}")
    if pixels is not None and tuple(pixels.shape) != (n,):
        raise ValueError(f"accumulate: pixels must be ({n},), got {tuple(pixels.shape)}")
    hip.check(hip.lib().stnerf_accumulate(vp, n, C_, stride if n > 1 else C_, hip.dptr(pixels, torch.int32, "pixels"), state.n_pixels,
                                          state.m2.shape[1], hip.dptr(state.mean, name="mean"), hip.dptr(state.m2, name="m2"),
                                          hip.dptr(state.count, torch.int32, "count"), hip.stream_ptr()), "stnerf_accumulate")
    return state


def accumulate_select(state: AccumulateState, min_spp: int, max_spp: int, tol: float) -> Tuple[Tensor, int]:
    """The pixels still to be sampled, ascending (stnerf_accumulate_select): count < min_spp, or count < max_spp and the variance
    of the mean of any of the V columns above tol^2 -- written m2 > tol2 * (float)(count * (count - 1)) with tol2 = tol * tol in
    fp32.  -> (pixels (n,) int32 on the device, n): n is a Python int, read back with one small D2H."""
    P = state.n_pixels
    if state._select is None:
        nbytes = hip.lib().stnerf_accumulate_select_workspace_bytes(P)
        if nbytes < 0:
            hip.check(int(nbytes), "stnerf_accumulate_select_workspace_bytes")
        dev = state.count.device
        state._select = (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                         torch.zeros(1, dtype=torch.int32, device=dev))
    work, out, n_out = state._select
    t = torch.tensor(float(tol), dtype=torch.float32)
    tol2 = float(t * t)
    hip.check(hip.lib().stnerf_accumulate_select(hip.dptr(state.m2, name="m2"), hip.dptr(state.count, torch.int32, "count"), P,
                                                 state.m2.shape[1], int(min_spp), int(max_spp), tol2, hip.dptr(out, torch.int32),
                                                 hip.dptr(n_out, torch.int32), hip.dptr(work, torch.uint8), work.numel(),
                                                 hip.stream_ptr()), "stnerf_accumulate_select")
    n = int(n_out.item())
    return out[:n].clone(), n      # (the buffer is the next call's too)


# ---------------------------------------------------------------------------------------- adaptive lattice frames
class LatticeState:
    """Per-pixel state of a lattice frame (include/stnerf.h: stnerf_lattice_begin): ``values`` (P,C), ``status`` (P,) uint8 --
    0 unknown, 1 rendered, 2 filled, 3 queued --, both zero at first; plus the flat bytes ``lattice_classify`` and the buffers
    ``lattice_select`` write (made on first use)."""

    def __init__(self, h: int, w: int, C_: int, device="cuda"):
        if h < 1 or w < 1 or C_ < 1:
            raise ValueError(f"lattice_state: need h, w >= 1 and C >= 1, got h={h}, w={w}, C={C_}")
        self.h, self.w = int(h), int(w)
        self.values = torch.zeros(h * w, C_, dtype=torch.float32, device=device)
        self.status = torch.zeros(h * w, dtype=torch.uint8, device=device)
        self._flat = self._select = None

    @property
    def n_pixels(self) -> int:
        return self.status.shape[0]


def lattice_state(h: int, w: int, C_: int, device="cuda") -> LatticeState:
    """A zeroed ``LatticeState`` for an h x w view of C floats per pixel."""
    return LatticeState(h, w, C_, device)


def lattice_begin(state: LatticeState, levels: int, force: Optional[Tensor] = None) -> LatticeState:
    """The first queue, IN PLACE (stnerf_lattice_begin): status 3 on the margin, where ``force`` -- None | (h, w) or (h w,) uint8 on
    the device -- is nonzero and on the points of the top lattice (stride 2^levels), 0 elsewhere.  -> state."""
    if force is not None:
        if force.numel() != state.n_pixels or tuple(force.shape) not in ((state.h, state.w), (state.n_pixels,)):
            raise ValueError(f"lattice_begin: force must be ({state.h},{state.w}) uint8, got {tuple(force.shape)}")
        force = force.reshape(-1)
    hip.check(hip.lib().stnerf_lattice_begin(state.h, state.w, int(levels), hip.dptr(force, torch.uint8, "force"),
                                             hip.dptr(state.status, torch.uint8, "status"), hip.stream_ptr()), "stnerf_lattice_begin")
    return state


def lattice_classify(state: LatticeState, levels: int, stride: int, tol: Tensor, exact: int = 1) -> LatticeState:
    """One level, IN PLACE (stnerf_lattice_classify): every covered pixel of status 0 whose cells of ``stride`` are all flat is filled
    from the first of them (status 2); another that is a point of the next lattice is queued (status 3).  tol: (C - exact,) float32
    on the device, the bound of every tested column; the last ``exact`` columns are compared with ==.  -> state."""
    C_ = state.values.shape[1]
    if tuple(tol.shape) != (C_ - int(exact),):
        raise ValueError(f"lattice_classify: tol must be ({C_ - int(exact)},), one bound per tested column, got {tuple(tol.shape)}")
    if state._flat is None:
        state._flat = torch.empty(state.n_pixels, dtype=torch.uint8, device=state.status.device)
    hip.check(hip.lib().stnerf_lattice_classify(hip.dptr(state.values, name="values"), hip.dptr(state.status, torch.uint8, "status"),
                                                state.h, state.w, C_, int(exact), int(levels), int(stride),
                                                hip.dptr(tol if tol.numel() else None, name="tol"), hip.dptr(state._flat, torch.uint8),
                                                state._flat.numel(), hip.stream_ptr()), "stnerf_lattice_classify")
    return state


def lattice_select(state: LatticeState) -> Tuple[Tensor, int]:
    """The queued pixels (status 3), ascending (stnerf_lattice_select).  -> (pixels (n,) int32 on the device, n): n is a Python
    int, read back with one small D2H."""
    P = state.n_pixels
    if state._select is None:
        nbytes = hip.lib().stnerf_lattice_select_workspace_bytes(P)
        if nbytes < 0:
            hip.check(int(nbytes), "stnerf_lattice_select_workspace_bytes")
        dev = state.status.device
        state._select = (torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                         torch.zeros(1, dtype=torch.int32, device=dev))
    work, out, n_out = state._select
    hip.check(hip.lib().stnerf_lattice_select(hip.dptr(state.status, torch.uint8, "status"), P, hip.dptr(out, torch.int32),
                                              hip.dptr(n_out, torch.int32), hip.dptr(work, torch.uint8), work.numel(),
                                              hip.stream_ptr()), "stnerf_lattice_select")
    n = int(n_out.item())
    return out[:n].clone(), n      # (the buffer is the next call's too)


def lattice_scatter(rows: Tensor, state: LatticeState, pixels: Tensor) -> LatticeState:
    """The rendered rows of some pixels, IN PLACE (stnerf_lattice_scatter): rows (n,C), a 2-D float32 device view with dense columns
    (any row stride), row i -> ``values[pixels[i]]`` and ``status[pixels[i]]`` = 1; pixels: a device int32 list that names a pixel
    at most once; an entry outside [0, P) is skipped.  -> state."""
    if rows.dim() != 2 or rows.shape[1] != state.values.shape[1]:
        raise ValueError(f"lattice_scatter: rows are {tuple(rows.shape)[1:]} floats wide, the state {state.values.shape[1]}")
    n, C_ = rows.shape
    if tuple(pixels.shape) != (n,):
        raise ValueError(f"lattice_scatter: pixels must be ({n},), got {tuple(pixels.shape)}")
    rp, stride = _mat(rows, "rows")
    hip.check(hip.lib().stnerf_lattice_scatter(rp, n, C_, stride if n > 1 else C_, hip.dptr(pixels, torch.int32, "pixels"), state.n_pixels,
                                               hip.dptr(state.values, name="values"), hip.dptr(state.status, torch.uint8, "status"),
                                               hip.stream_ptr()), "stnerf_lattice_scatter")
    return state


# ---------------------------------------------------------------------------------------- reprojection into a nearby view
def world_to_camera(T) -> "np.ndarray":
    """Wd (3,4) float32 of a camera-to-world pose T (4,4): the inverse taken in fp64 on the host, rounded once (include/stnerf.h)."""
    import numpy as np
    Tm = np.asarray(torch.as_tensor(T).detach().cpu().numpy(), dtype=np.float64).reshape(4, 4)
    return np.ascontiguousarray(np.linalg.inv(Tm)[:3, :4].astype(np.float32))


def reproject_keys(h_d: int, w_d: int, device="cuda") -> Tensor:
    """The splat target of an h_d x w_d view, all empty: (h_d w_d,) int64 holding the all-ones 64-bit key."""
    return torch.full((h_d * w_d,), -1, dtype=torch.int64, device=device)


def reproject_splat(keys: Tensor, K_s: Tensor, T_s: Tensor, h_s: int, w_s: int, t_src: Tensor, id_base: int, K_d: Tensor, T_d: Tensor,
                    h_d: int, w_d: int, z_min: float = 1e-6) -> Tensor:
    """Splat the rows of one source view into ``keys`` IN PLACE (stnerf_reproject_splat): row q of t_src (n,), n <= h_s w_s, is
    the ray parameter of pixel q of the source; the nearest surface wins a destination pixel, on a tie the lower id.  -> keys."""
    import numpy as np
    if t_src.dim() != 1:
        raise ValueError(f"reproject_splat: t must be (n,), got {tuple(t_src.shape)}")
    kinv = torch.inverse(K_s.detach().to("cpu", torch.float32)).contiguous()   # as generate_rays takes it
    Ts = torch.as_tensor(T_s, dtype=torch.float32).detach().cpu().contiguous()
    Kd = K_d.detach().to("cpu", torch.float32).contiguous()
    Td = torch.as_tensor(T_d, dtype=torch.float32).detach().cpu().contiguous()
    Wd = world_to_camera(Td)
    od = np.ascontiguousarray(Td.numpy()[:3, 3])
    hip.check(hip.lib().stnerf_reproject_splat((C.c_float * 9)(*kinv.reshape(-1).tolist()), (C.c_float * 16)(*Ts.reshape(-1).tolist()),
                                               h_s, w_s, hip.dptr(t_src, name="t"), t_src.shape[0], int(id_base),
                                               (C.c_float * 9)(*Kd.reshape(-1).tolist()), (C.c_float * 12)(*Wd.reshape(-1).tolist()),
                                               (C.c_float * 3)(*od.tolist()), h_d, w_d, float(z_min), hip.dptr(keys, torch.int64, "keys"),
                                               hip.stream_ptr()), "stnerf_reproject_splat")
    return keys


def reproject_resolve(keys: Tensor, h_d: int, w_d: int, rel: float, values: Sequence[Tensor], out=None):
    """Resolve splatted keys (stnerf_reproject_resolve): values = the sources' rows, (n_s, C) float32 device views with dense
    columns, in the order of their id bases.  -> (values (h_d w_d, C), t (h_d w_d,), src (h_d w_d,) int32); a hole has zeros, a NaN
    t and src = -1.  ``out``: the three buffers to write instead of new ones."""
    if not 1 <= len(values) <= hip.REPROJECT_MAX_SOURCES:
        raise ValueError(f"reproject_resolve: {len(values)} sources (1..{hip.REPROJECT_MAX_SOURCES})")
    C_ = values[0].shape[1] if values[0].dim() == 2 else 0
    table = (hip.ReprojectSource * len(values))()
    for i, v in enumerate(values):
        if v.dim() != 2 or v.shape[1] != C_:
            raise ValueError(f"reproject_resolve: every source must be (n, {C_}), got {tuple(v.shape)}")
        vp, stride = _mat(v, "values")
        table[i].values, table[i].row_stride, table[i].n = vp.value, (stride if v.shape[0] > 1 else C_), v.shape[0]
    P = h_d * w_d
    dev = keys.device
    vals, t, src = out if out is not None else (torch.empty(P, C_, dtype=torch.float32, device=dev),
                                                torch.empty(P, dtype=torch.float32, device=dev),
                                                torch.empty(P, dtype=torch.int32, device=dev))
    hip.check(hip.lib().stnerf_reproject_resolve(hip.dptr(keys, torch.int64, "keys"), h_d, w_d, float(rel), table, len(values), C_,
                                                 hip.dptr(vals, name="values_out"), hip.dptr(t, name="t_out"),
                                                 hip.dptr(src, torch.int32, "src"), hip.stream_ptr()), "stnerf_reproject_resolve")
    return vals, t, src


def reproject_holes(src: Tensor) -> Tuple[Tensor, int]:
    """The pixels with src < 0, ascending (stnerf_reproject_holes).  -> (holes (n,) int32 on the device, n): n is a Python int,
    read back with one small D2H."""
    P = src.shape[0]
    nbytes = hip.lib().stnerf_reproject_holes_workspace_bytes(P)
    if nbytes < 0:
        hip.check(int(nbytes), "stnerf_reproject_holes_workspace_bytes")
    dev = src.device
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(P, dtype=torch.int32, device=dev)
    n_out = torch.zeros(1, dtype=torch.int32, device=dev)
    hip.check(hip.lib().stnerf_reproject_holes(hip.dptr(src, torch.int32, "src"), P, hip.dptr(out, torch.int32), hip.dptr(n_out, torch.int32),
                                               hip.dptr(work, torch.uint8), work.numel(), hip.stream_ptr()), "stnerf_reproject_holes")
    n = int(n_out.item())
    return out[:n], n


def reproject(sources, K_d: Tensor, T_d: Tensor, h_d: int, w_d: int, rel: float, z_min: float = 1e-6):
    """Warp the rows of up to four source views into the view (K_d, T_d, h_d, w_d): splat every source, resolve, list the holes.
    sources: a list of (K, T, h, w, values (n,C), t (n,)) -- row q belongs to pixel q of its view, t is its ray parameter (NaN or
    <= 0: absent).  -> (values (h_d w_d, C), t (h_d w_d,), src (h_d w_d,) int32, holes (n_holes,) int32 ascending, n_holes).
    src is the id of the row a pixel took: its row number plus the row counts of the sources before it; -1 for a hole."""
    if not 1 <= len(sources) <= hip.REPROJECT_MAX_SOURCES:
        raise ValueError(f"reproject: {len(sources)} sources (1..{hip.REPROJECT_MAX_SOURCES})")
    keys = reproject_keys(h_d, w_d, sources[0][4].device)
    base = 0
    for (K_s, T_s, h_s, w_s, values, t_src) in sources:
        if values.dim() != 2 or tuple(t_src.shape) != (values.shape[0],):
            raise ValueError(f"reproject: a source needs values (n,C) and t (n,), got {tuple(values.shape)} and {tuple(t_src.shape)}")
        reproject_splat(keys, K_s, T_s, h_s, w_s, t_src, base, K_d, T_d, h_d, w_d, z_min)
        base += values.shape[0]
    vals, t, src = reproject_resolve(keys, h_d, w_d, rel, [s[4] for s in sources])
    holes, n_holes = reproject_holes(src)
    return vals, t, src, holes, n_holes


# ---------------------------------------------------------------------------------------- 8(f)4: training GEMMs
def _mat(t: Tensor, name: str, vec: bool = False):
    """(pointer, row stride) of a 2-D fp32 device view whose columns are dense; `vec`: read with 16-byte vectors."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected a 2-D float32 view with dense columns, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    if vec and (t.stride(0) % 4 or t.data_ptr() % 16):
        raise ValueError(f"{name}: rows must be 16-byte aligned (row stride {t.stride(0)} floats, pointer % 16 = {t.data_ptr() % 16})")
    return C.c_void_p(t.data_ptr()), t.stride(0)


def train_linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], y: Tensor, relu: bool) -> Tensor:
    """y (m,n) = act(x (m,k) @ w (n,k).T + bias): stnerf_train_linear_fwd (f32 MFMA).  x / w: views into padded storage."""
    (m, k), n = x.shape, w.shape[0]
    xp, ldx = _mat(x, "x", True)
    wp, ldw = _mat(w, "w", True)
    yp, ldy = _mat(y, "y")
    if w.shape[1] != k or tuple(y.shape) != (m, n):
        raise ValueError(f"train_linear_fwd: x {tuple(x.shape)}, w {tuple(w.shape)}, y {tuple(y.shape)}")
    hip.check(hip.lib().stnerf_train_linear_fwd(xp, ldx, wp, ldw, hip.dptr(bias, name="bias"), m, n, k, int(relu), yp, ldy,
                                                hip.stream_ptr()), "stnerf_train_linear_fwd")
    return y


def train_linear_dx(dy: Tensor, w: Tensor, dx: Tensor, mask: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """dx (m,k) (+)= (dy (m,n) @ w (n,k)) * (mask > 0): stnerf_train_linear_dx."""
    (m, n), k = dy.shape, w.shape[1]
    dp, lddy = _mat(dy, "dy", True)
    wp, ldw = _mat(w, "w", True)
    xp, lddx = _mat(dx, "dx")
    mp, ldm = _mat(mask, "mask") if mask is not None else (C.c_void_p(0), 0)
    if w.shape[0] != n or tuple(dx.shape) != (m, k) or (mask is not None and tuple(mask.shape) != (m, k)):
        raise ValueError(f"train_linear_dx: dy {tuple(dy.shape)}, w {tuple(w.shape)}, dx {tuple(dx.shape)}")
    hip.check(hip.lib().stnerf_train_linear_dx(dp, lddy, wp, ldw, m, n, k, mp, ldm, int(accumulate), xp, lddx, hip.stream_ptr()),
              "stnerf_train_linear_dx")
    return dx


_DW_WORKSPACE: dict = {}


def train_linear_dw(dy: Tensor, x: Tensor, dw: Tensor, db: Optional[Tensor], accumulate: bool) -> None:
    """dw (n,k) (+)= dy (m,n).T @ x (m,k); db (n,) (+)= dy.sum(0): stnerf_train_linear_dw (deterministic split reduction)."""
    (m, n), k = dy.shape, x.shape[1]
    dp, lddy = _mat(dy, "dy", True)
    xp, ldx = _mat(x, "x", True)
    wp, lddw = _mat(dw, "dw")
    if x.shape[0] != m or tuple(dw.shape) != (n, k) or (db is not None and tuple(db.shape) != (n,)):
        raise ValueError(f"train_linear_dw: dy {tuple(dy.shape)}, x {tuple(x.shape)}, dw {tuple(dw.shape)}")
    ws = _dw_workspace(int(hip.lib().stnerf_train_dw_workspace_bytes(m, n, k)), dy.device)
    hip.check(hip.lib().stnerf_train_linear_dw(dp, lddy, xp, ldx, m, n, k, wp, lddw, hip.dptr(db, name="db"), int(accumulate),
                                               hip.dptr(ws, torch.uint8, "workspace"), ws.numel(), hip.stream_ptr()), "stnerf_train_linear_dw")


def free_workspaces() -> None:
    """Drop the cached weight-gradient workspaces (tens of MB per (device, stream) that ran a backward); they are re-created on demand."""
    _DW_WORKSPACE.clear()


def _dw_workspace(need: int, device) -> Tensor:
    # one workspace per device and stream, grown on demand (a backward's calls run in order on one stream, so the partial tiles of
    # one may overwrite the previous call's -- ADVICE r04).  ASSUMES one host thread per stream: two threads that enqueue backwards on
    # the SAME stream would share the partial tiles (the trainer is single-threaded, one process per GPU).  The cache only
    # grows; free_workspaces() releases it.
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _DW_WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        ws = _DW_WORKSPACE[key] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=device)
    return ws


DW_BATCH_MAX = 16


def _dw_problems(layers):
    """-> (the stnerf_dw_problem array of `layers`, m)"""
    if len(layers) > DW_BATCH_MAX:
        raise ValueError(f"train_dw_batch: {len(layers)} layers, at most {DW_BATCH_MAX}")
    m = layers[0][0].shape[0]
    arr = (hip.DwProblem * len(layers))()
    for i, (dy, x, dw, db) in enumerate(layers):
        n, k = dy.shape[1], x.shape[1]
        dp, lddy = _mat(dy, f"dy[{i}]", True)
        xp, ldx = _mat(x, f"x[{i}]", True)
        wp, lddw = _mat(dw, f"dw[{i}]")
        if dy.shape[0] != m or x.shape[0] != m or tuple(dw.shape) != (n, k) or (db is not None and tuple(db.shape) != (n,)):
            raise ValueError(f"train_dw_batch: layer {i}: dy {tuple(dy.shape)}, x {tuple(x.shape)}, dw {tuple(dw.shape)}, m = {m}")
        bp = hip.dptr(db, name=f"db[{i}]")
        arr[i] = hip.DwProblem(dp.value, lddy, xp.value, ldx, wp.value, lddw, bp.value if bp is not None else None, n, k)
    return arr, m


def train_dw_batch_bundles(layers: Sequence[Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]]) -> Tuple[int, int, int]:
    """How ``train_dw_batch`` would run `layers` (stnerf_train_dw_batch_plan, host arithmetic): the number of (split-bf16 2 x 2,
    f32 2 x 2, shared-input) LDS bundles of the plan."""
    arr, m = _dw_problems(layers)
    out = (C.c_int32 * 3)()
    hip.check(hip.lib().stnerf_train_dw_batch_plan(arr, len(layers), m, out), "stnerf_train_dw_batch_plan")
    return int(out[0]), int(out[1]), int(out[2])


def train_dw_batch(layers: Sequence[Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]], accumulate: bool) -> None:
    """For every (dy (m,n), x (m,k), dw (n,k), db (n,) | None) of `layers` (the same m): dw (+)= dy.T @ x, db (+)= dy.sum(0) --
    stnerf_train_dw_batch: all weight and bias gradients of a network in one launch and one deterministic reduction."""
    if not layers:
        return
    arr, m = _dw_problems(layers)
    need = int(hip.lib().stnerf_train_dw_batch_workspace_bytes(arr, len(layers), m))
    if need < 0:
        hip.check(need, "stnerf_train_dw_batch_workspace_bytes")
    ws = _dw_workspace(need, layers[0][0].device)
    hip.check(hip.lib().stnerf_train_dw_batch(arr, len(layers), m, int(accumulate), hip.dptr(ws, torch.uint8, "workspace"), ws.numel(),
                                              hip.stream_ptr()), "stnerf_train_dw_batch")


def train_encode(x: Tensor, y: Tensor, n_freq: int, include_input: bool = True, rows_per_src: int = 1, relu: bool = False,
                 lerp_col: int = -1) -> Tensor:
    """Positional encoding of x (src, dim) into the columns of the view y (rows, dim (include_input + 2 n_freq)):
    stnerf_train_encode (rows = src * rows_per_src)."""
    xp, ldx = _mat(x, "x")
    yp, ldy = _mat(y, "y")
    dim, rows = x.shape[1], y.shape[0]
    if y.shape[1] != dim * (int(include_input) + 2 * n_freq) or rows != x.shape[0] * rows_per_src:
        raise ValueError(f"train_encode: x {tuple(x.shape)} -> y {tuple(y.shape)}")
    hip.check(hip.lib().stnerf_train_encode(xp, ldx, dim, n_freq, int(include_input), rows, rows_per_src, int(relu), lerp_col, yp, ldy, 0,
                                            hip.stream_ptr()), "stnerf_train_encode")
    return y


def train_encode_bwd(x: Tensor, dy: Tensor, dx: Tensor, n_freq: int, include_input: bool = True, accumulate: bool = False) -> Tensor:
    """dx (rows, dim_out) (+)= d enc / d x . dy for the first dim_out = dx.shape[1] input columns: stnerf_train_encode_bwd."""
    xp, ldx = _mat(x, "x")
    dp, lddy = _mat(dy, "dy")
    op, lddx = _mat(dx, "dx")
    dim, rows = x.shape[1], x.shape[0]
    if dy.shape[1] != dim * (int(include_input) + 2 * n_freq) or dy.shape[0] != rows or dx.shape[0] != rows or dx.shape[1] > dim:
        raise ValueError(f"train_encode_bwd: x {tuple(x.shape)}, dy {tuple(dy.shape)}, dx {tuple(dx.shape)}")
    hip.check(hip.lib().stnerf_train_encode_bwd(xp, ldx, dim, n_freq, int(include_input), rows, dp, lddy, 0, dx.shape[1], int(accumulate),
                                                op, lddx, hip.stream_ptr()), "stnerf_train_encode_bwd")
    return dx


# ---------------------------------------------------------------------------------------- fused training launches (csrc/train_wave.hip)
def _matrix_list(mats: Sequence[Tensor], name: str):
    ptrs = (C.c_void_p * len(mats))()
    lds = (C.c_int32 * len(mats))()
    for i, m in enumerate(mats):
        p, ld = _mat(m, f"{name}[{i}]")
        ptrs[i], lds[i] = p.value, ld
    return ptrs, lds


def _bit_planes(bits: Tensor, rows: int):
    """(pointer, stage stride in words) of the ReLU bit planes: int32 (8, rows, 8), possibly a row range ``planes[:, a:b]`` of a larger
    launch's planes (rows and words dense, any stage stride)."""
    if not bits.is_cuda or bits.dtype != torch.int32 or tuple(bits.shape) != (8, rows, 8) or bits.stride(2) != 1 or bits.stride(1) != 8:
        raise ValueError(f"relu_bits must be a device int32 (8, {rows}, 8) with dense rows, got {bits.dtype} {tuple(bits.shape)} {bits.stride()}")
    return C.c_void_p(bits.data_ptr()), bits.stride(0)


def train_spacenet_fwd(net: PackedNet, xyz: Tensor, dirs: Tensor, times: Optional[Tensor], raw: Tensor, acts: Sequence[Tensor],
                       pe: Tensor, relu_bits: Optional[Tensor] = None) -> None:
    """The stage kernel of the network's arithmetic (exact f32: stnerf_train_spacenet_fwd; split bf16: ..._bf16x3) on one SpaceNet,
    every ray, writing each layer's input as it goes: acts[0..6] (rows, 256), acts[7] (rows, 128), pe (rows, 64), rows = n * ns in
    (ray, sample) order -- views into padded row-major storage -- and relu_bits (8, rows, 8) int32: the ReLU masks as bit planes.
    xyz (n,ns,3), dirs (n,3), times (n,) | None, raw (n,ns,4) out."""
    entry = "stnerf_train_spacenet_fwd" if net.precision == "fp32" else "stnerf_train_spacenet_fwd_bf16x3"
    n, ns = xyz.shape[0], xyz.shape[1]
    xp, xs = _strided_view_ptr(xyz, (ns, 3), "xyz")
    rp, rs = _strided_view_ptr(raw, (ns, 4), "raw")
    dp, ds = _strided_view_ptr(dirs, (3,), "dirs")
    tp, ts = _strided_view_ptr(times.reshape(n), (), "times") if times is not None else (C.c_void_p(0), 0)
    ptrs, lds = _matrix_list(acts, "acts")
    pp, ldp = _mat(pe, "pe")
    bp, bstride = _bit_planes(relu_bits, n * ns) if relu_bits is not None else (C.c_void_p(0), 0)
    queue = torch.zeros(1, dtype=torch.int32, device=xyz.device)
    ray_bias = torch.empty(n, 128, dtype=torch.float32, device=xyz.device)
    hip.check(getattr(hip.lib(), entry)(net.kind, hip.dptr(net.blob), n, ns, xp, xs, dp, ds, tp, ts, rp, rs, ptrs, lds, pp, ldp,
                                        bp, bstride, hip.dptr(queue, torch.int32), hip.dptr(ray_bias), hip.stream_ptr()), entry)


def train_spacenet_dx(wt: Tensor, offsets: Sequence[int], d_raw: Tensor, relu_bits: Tensor, dys: Sequence[Tensor], dpe: Optional[Tensor]) -> None:
    """The backward chain through one SpaceNet's layers (stnerf_train_spacenet_dx): d_raw (rows,4) -> dys[0..7] (the layers'
    pre-activation gradients, widths 256 x 7, 128) and, if given, dpe (rows,64) = dLoss / d PE(pos).  relu_bits (8, rows, 8) int32:
    the masks ``train_spacenet_fwd`` wrote for these rows.  wt / offsets: the transposed weight sections
    (stnerf_amd.modeling.autograd.transposed_spacenet)."""
    rows = d_raw.shape[0]
    bp, bstride = _bit_planes(relu_bits, rows)
    yp, yld = _matrix_list(dys, "dys")
    off = (C.c_uint32 * 10)(*[int(o) for o in offsets])
    pp, ldp = _mat(dpe, "dpe") if dpe is not None else (C.c_void_p(0), 0)
    hip.check(hip.lib().stnerf_train_spacenet_dx(hip.dptr(wt, name="wt"), off, hip.dptr(d_raw, name="d_raw"), rows,
                                                 bp, bstride, yp, yld, pp, ldp, hip.stream_ptr()),
              "stnerf_train_spacenet_dx")


def pack_dx_bf16x3(kind: int, weights: Sequence[Tensor], with_dpos: bool) -> Tensor:
    """The split-bf16 backward chain's weights in one blob (stnerf_pack_dx_bf16x3_device): the network's 10 weight tensors in reference
    layout (device, fp32) -> a 1 KB-aligned uint8 device tensor.  with_dpos: with the two half passes towards PE(pos)."""
    lib = hip.lib()
    nbytes = lib.stnerf_packed_bytes_dx_bf16x3(kind, int(with_dpos))
    if nbytes < 0:
        hip.check(int(nbytes), "stnerf_packed_bytes_dx_bf16x3")
    ws = [w.detach().to(torch.float32).contiguous() for w in weights]
    if not all(w.is_cuda for w in ws):
        raise ValueError("pack_dx_bf16x3 packs on the device: the weights must be CUDA tensors")
    dev = ws[0].device
    raw = torch.empty(nbytes + 1024, dtype=torch.uint8, device=dev)
    off = (-raw.data_ptr()) % 1024
    blob = raw[off:off + nbytes]
    wp = (C.c_void_p * len(ws))(*(w.data_ptr() for w in ws))
    with torch.cuda.device(dev):
        hip.check(lib.stnerf_pack_dx_bf16x3_device(kind, wp, len(ws), int(with_dpos), C.c_void_p(blob.data_ptr()), nbytes, hip.stream_ptr()),
                  "stnerf_pack_dx_bf16x3_device")
    return blob


def train_spacenet_dx_bf16x3(blob: Tensor, d_raw: Tensor, relu_bits: Tensor, dys: Sequence[Tensor], dpe: Optional[Tensor],
                             dpe_skip: Optional[Tensor]) -> None:
    """``train_spacenet_dx`` in split bf16 (stnerf_train_spacenet_dx_bf16x3): blob = ``pack_dx_bf16x3``; dLoss / d PE(pos) leaves as
    dpe + dpe_skip (both (rows,64)) when the blob was packed with_dpos, else both None."""
    rows = d_raw.shape[0]
    bp, bstride = _bit_planes(relu_bits, rows)
    yp, yld = _matrix_list(dys, "dys")
    pp, ldp = _mat(dpe, "dpe") if dpe is not None else (C.c_void_p(0), 0)
    sp, lds_ = _mat(dpe_skip, "dpe_skip") if dpe_skip is not None else (C.c_void_p(0), 0)
    hip.check(hip.lib().stnerf_train_spacenet_dx_bf16x3(C.c_void_p(blob.data_ptr()), int(dpe is not None), hip.dptr(d_raw, name="d_raw"), rows,
                                                        bp, bstride, yp, yld, pp, ldp, sp, lds_, hip.stream_ptr()),
              "stnerf_train_spacenet_dx_bf16x3")


def _motion_bit_planes(bits: Tensor, rows: int):
    """(pointer, stage stride in words) of a MotionNet's ReLU bit planes: int32 (5, rows, 4), possibly a row range of a larger launch's."""
    if not bits.is_cuda or bits.dtype != torch.int32 or tuple(bits.shape) != (5, rows, 4) or bits.stride(2) != 1 or bits.stride(1) != 4:
        raise ValueError(f"relu_bits must be a device int32 (5, {rows}, 4) with dense rows, got {bits.dtype} {tuple(bits.shape)} {bits.stride()}")
    return C.c_void_p(bits.data_ptr()), bits.stride(0)


def train_motionnet_fwd(net: PackedNet, xt: Tensor, flow: Tensor, enc: Tensor, acts: Sequence[Tensor], relu_bits: Tensor,
                        plain_time: bool = False) -> None:
    """flow (rows,3) = MotionNet(xt (rows,4) = [xyz | frame id]) with the inference kernels' exact-f32 arithmetic, writing the staged
    encoding enc (rows, >= 88), the five post-ReLU outputs acts[0..4] (rows,128) -- views into padded row-major storage -- and their
    masks as bit planes relu_bits (5, rows, 4) int32 (stnerf_train_motionnet_fwd)."""
    if net.kind != hip.NET_MOTION or net.precision != "fp32":
        raise ValueError("train_motionnet_fwd wants an exact-f32 packed MotionNet")
    rows = xt.shape[0]
    if tuple(xt.shape) != (rows, 4) or not xt.is_contiguous() or tuple(flow.shape) != (rows, 3) or not flow.is_contiguous() or len(acts) != 5:
        raise ValueError(f"train_motionnet_fwd: xt {tuple(xt.shape)}, flow {tuple(flow.shape)}, {len(acts)} activation matrices")
    ap, ald = _matrix_list(acts, "acts")
    ep, lde = _mat(enc, "enc", True)
    if enc.shape != (rows, enc.shape[1]) or enc.shape[1] < 88 or any(tuple(m.shape) != (rows, 128) for m in acts):
        raise ValueError("train_motionnet_fwd: enc needs >= 88 columns, the activation matrices 128, one row per sample")
    bp, bstride = _motion_bit_planes(relu_bits, rows)
    hip.check(hip.lib().stnerf_train_motionnet_fwd(hip.dptr(net.blob), hip.dptr(xt, name="xt"), rows, hip.MOTION_PLAIN_TIME if plain_time else 0,
                                                   hip.dptr(flow, name="flow"), ep, lde, ap, ald, bp, bstride, hip.stream_ptr()),
              "stnerf_train_motionnet_fwd")


def train_motionnet_dx(wt: Tensor, offsets: Sequence[int], d_flow: Tensor, relu_bits: Tensor, dys: Sequence[Tensor], denc: Optional[Tensor]) -> None:
    """The backward chain through one MotionNet (stnerf_train_motionnet_dx): d_flow (rows,3) as a view of (rows,4) storage -> dys[0..4]
    (rows,128), the layers' pre-activation gradients, and, if given, denc (rows, >= 96) = dLoss / d encoding.  wt / offsets:
    stnerf_amd.modeling.autograd.transposed_motionnet."""
    rows = d_flow.shape[0]
    dp, ldf = _mat(d_flow, "d_flow", True)
    if d_flow.shape[1] != 3 or ldf != 4 or len(dys) != 5 or any(tuple(m.shape) != (rows, 128) for m in dys):
        raise ValueError(f"train_motionnet_dx: d_flow {tuple(d_flow.shape)} (row stride {ldf}), {len(dys)} gradient matrices")
    bp, bstride = _motion_bit_planes(relu_bits, rows)
    yp, yld = _matrix_list(dys, "dys")
    off = (C.c_uint32 * 6)(*[int(o) for o in offsets])
    pp, ldp = _mat(denc, "denc", True) if denc is not None else (C.c_void_p(0), 0)
    if denc is not None and (denc.shape[0] != rows or denc.shape[1] < 96):
        raise ValueError(f"train_motionnet_dx: denc {tuple(denc.shape)} needs {rows} rows of >= 96 columns")
    hip.check(hip.lib().stnerf_train_motionnet_dx(hip.dptr(wt, name="wt"), off, dp, rows, bp, bstride, yp, yld, pp, ldp, hip.stream_ptr()),
              "stnerf_train_motionnet_dx")


def pack_transposed(sections: Sequence[Tuple[Tensor, int]], dst: Tensor) -> List[int]:
    """The A operands of the fused backward chains in one launch (stnerf_pack_transposed): for every (W (out, in) fp32 device view with
    dense columns, n_pad) a section [out / 4][n_pad][4] of `dst` (n_pad = 0: W copied as it is), packed back to back from offset 0.
    -> the sections' float offsets."""
    arr = (hip.TransposeSection * len(sections))()
    offsets, off = [], 0
    for i, (w, n_pad) in enumerate(sections):
        wp, ldw = _mat(w, f"w[{i}]")
        out, k = w.shape
        arr[i] = hip.TransposeSection(wp.value, ldw, off, out, k, n_pad)
        offsets.append(off)
        off += out * (n_pad if n_pad else k)
    if dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() < off:
        raise ValueError(f"pack_transposed: the destination needs {off} contiguous fp32 values")
    hip.check(hip.lib().stnerf_pack_transposed(arr, len(sections), hip.dptr(dst, name="dst"), dst.numel(), hip.stream_ptr()),
              "stnerf_pack_transposed")
    return offsets
