"""Per-pose rendering with the reference's post-processing.

Mirrors ``LayeredNeuralRenderer.render_pose`` (render/layered_neural_renderer.py:364-391) without the
dataset object: rays are generated on the device from (K, pose) -- no CPU ray tensor, no 75 MB H2D per
frame -- and the images stay on the device until the caller moves them.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from stnerf_amd.parallel import render_view, total_layers


def render_pose(model, pose, K, height: int, width: int, layer_frame_pair: Sequence[Tuple[int, float]], far: float,
                density_threshold: float = 0, bkgd_density_threshold: float = 0, device="cuda", scene_passes: bool = False,
                occluder=None, occluder_stops: bool = False, accumulate=None, lens=None, reproject=None, lattice=None, deep=None):
    """-> color (H,W,3), depth (H,W,1), color_layer [l x (H,W,3)], depth_layer [l x (H,W,1)].

    ``layer_frame_pair``: (layer_id, frame_id) pairs as in data/datasets/ray_dataset.py:276-281.
    Depth post-processing as in the reference: negative mixed depth -> 0, then / far (:382-383); the
    per-layer depths are divided by far; their ``depth_1[depth < 0] = 0`` (:388) tests the already
    clamped mixed depth and therefore never fires -- reproduced as a no-op.

    One process per GPU under an initialised torch.distributed group: every rank generates and renders its interleaved
    row stripes of the view only (``model.shard_views = True``: opt-in), one all-gather rebuilds the images this function
    returns on every rank -- gather mode "fine": 6 + 5 l floats per ray instead of the whole 5-tuple's 11 + 10 l
    (stnerf_amd.parallel.render_view); the return value is the single-GPU one, bit for bit.

    ``scene_passes``: a fifth element, the in-scene layer passes (``LayeredRFRender.render_rays_scene``) as a dict of per-layer
    image lists on the device: ``color_scene`` (H,W,3) premultiplied, ``alpha_scene`` (H,W,1), ``depth_scene`` (H,W,1) = the
    weighted depth / far, not clamped.  Their sums over the layers are the mixed colour, alpha and (unclamped) depth.  One rank
    only.

    ``occluder`` = (rgba (H,W,4), depth (H,W)): a depth-tested occluder in the scene -- a CG prop, a title card, a plate with a
    z-buffer (``LayeredRFRender.render_rays_occluded``).  rgba: straight (not premultiplied) colour and
    coverage; ``depth`` is in RAY-PARAMETER units, those of the depth outputs before the division by far
    (``ops.ray_parameter`` converts a camera-space z-buffer); a pixel with alpha <= 0 or a depth that is not finite has no
    occluder.  The fifth element is returned as with ``scene_passes`` (the plain passes come with it either way) and gains
    ``color_occluded`` (H,W,3), ``alpha_occluded``, ``depth_occluded`` (H,W,1; weighted depth / far, not clamped) -- the mixed image
    with the occluder in it --, the per-layer lists ``color_scene_occluded`` / ``alpha_scene_occluded`` / ``depth_scene_occluded`` --
    every layer's share of it -- and ``occluder_share`` = (colour (H,W,3), alpha (H,W,1), depth (H,W,1) / far), the occluder's own
    premultiplied share.  ``occluder_stops``: opaque pixels also stop early ray termination at their depth
    (``render_rays_occluded(stops=True)``: it needs ``model.set_termination``).  One rank only.

    ``accumulate`` = an ``stnerf_amd.accumulate.AccumulateSpec`` (or the dict of its arguments): the frame is the per-pixel mean
    of several passes -- anti-aliasing, motion blur, adaptive samples per pixel (``parallel.render_view_accumulated``; DESIGN.md
    section 7).  The depth post-processing above is applied to the means, and a fifth element ``stats`` is returned: ``spp``
    (H,W) int32, ``variance`` (H,W,3) of the mixed colour's mean, ``passes``, ``rays_rendered``.  It does not combine with
    ``scene_passes`` or an occluder (ValueError).  One rank only.

    ``lens`` = an ``stnerf_amd.lens.Lens`` (or the dict of its arguments): the camera's lens.  Its distortion
    bends the rays of this frame so that it lines up with a plate shot through that lens -- nothing is resampled, and scene passes,
    an occluder and the caches work as without it.  Its ``aperture`` gives depth of field and needs ``accumulate`` (ValueError
    without): every pass then starts its rays at another point of the lens.  One rank only.

    ``reproject`` = (spec, plates): the background of this frame is warped from the key plates of nearby views
    (``stnerf_amd.reproject``: a ``ReprojectSpec`` or the dict of its arguments, a list of ``BackgroundPlate``), only its holes
    are rendered, and the finished plate is composited into the scene as an occluder with layer 0 hidden
    (``parallel.render_view_reprojected``).  color and depth are the occluded mixed image's; the per-layer
    lists are the render's own (layer 0 was hidden in it).  A fifth element ``stats`` is returned: ``holes``,
    ``reused``, ``rays_background``, ``keys``, and ``passes`` = the dict an occluder returns.  It does not combine with
    ``accumulate``, an occluder of the caller's or an enabled lens (ValueError).  Approximate; inference only; one rank only.
    With ``ReprojectSpec(exclusive=True)`` no hole is rendered separately and layer 0 is not hidden: one render call evaluates the
    background exactly on the rays whose plate row is absent (a per-ray background mask) and takes the plate on the others;
    ``holes`` = ``rays_background`` = those rays.

    ``lattice`` = an ``stnerf_amd.lattice.LatticeSpec`` (or the dict of its arguments): the frame is rendered on a sparse lattice of
    pixels, refined where the corners of a cell disagree and interpolated where they agree
    (``parallel.render_view_lattice``).  The depth post-processing above is applied to the finished state, and
    a fifth element ``stats`` is returned: ``rendered``, ``filled``, ``forced``, ``margin``, ``rays_per_level`` and ``status`` (H,W)
    uint8 (1 rendered, 2 filled).  A distorting ``lens`` passes through; it does not combine with ``accumulate``, ``reproject``,
    ``scene_passes``, an occluder or a lens with an aperture (ValueError).  Approximate; inference only; one rank only.
    ``deep`` = an ``stnerf_amd.DeepSpec``: the fifth element is returned as with ``scene_passes`` and gains ``deep``, the frame's
    ``stnerf_amd.DeepFrame`` (H x W pixels, ``far`` set): the per-pixel list of the final stage's weighted samples, on which
    ``DeepFrame.composite`` puts any number of depth-tested elements after the render.  With an occluder the
    deep frame is of the scene without it.  It does not combine with ``accumulate``, ``lattice`` or ``reproject`` (ValueError: those
    frames are not one sample list per pixel) nor with ``occluder_stops``.  Inference only; one rank only."""
    if deep is not None:
        for name, value in (("accumulate", accumulate), ("lattice", lattice), ("reproject", reproject)):
            if value is not None:
                raise ValueError(f"render_pose(deep=...) with {name}=: such a frame is not one sample list per pixel; render the deep "
                                 f"frame without {name}=")
    if lattice is not None:
        from stnerf_amd.parallel import render_view_lattice
        frame_ids = [0.0] * total_layers(model)
        for layer_id, frame_id in layer_frame_pair:
            frame_ids[layer_id] = float(frame_id)
        (stage2, _, stage2_layer, _, _), stats = render_view_lattice(
            model, torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(pose, dtype=torch.float32), height, width, frame_ids,
            lattice, density_threshold, bkgd_density_threshold, device=device, scene=bool(scene_passes), occluder=occluder,
            accumulate=accumulate, reproject=reproject, **(dict(lens=lens) if lens is not None else {}))
        stats = dict(stats, status=stats["status"].reshape(height, width))
        return (stage2[0].reshape(height, width, 3), stage2[1].reshape(height, width, 1).clamp_min(0) / far,
                [t[0].reshape(height, width, 3) for t in stage2_layer], [t[1].reshape(height, width, 1) / far for t in stage2_layer],
                stats)
    if reproject is not None:
        from stnerf_amd.parallel import render_view_reprojected
        if accumulate is not None:
            raise ValueError("render_pose(reproject=...) with accumulate=: plates for the passes of a progressive frame are out of "
                             "scope; render the frame with one of the two")
        if scene_passes:
            raise ValueError("render_pose(reproject=...) with scene_passes: layer 0 is hidden in a reprojected frame, so its pass "
                             "would be empty; the passes of the frame are in stats[\"passes\"]")
        spec, plates = reproject
        frame_ids = [0.0] * total_layers(model)
        for layer_id, frame_id in layer_frame_pair:
            frame_ids[layer_id] = float(frame_id)
        out = render_view_reprojected(model, torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(pose, dtype=torch.float32), height,
                                      width, frame_ids, plates, spec, density_threshold, bkgd_density_threshold, device=device,
                                      **(dict(occluder=occluder) if occluder is not None else {}),
                                      **(dict(lens=lens) if lens is not None else {}))
        (stage2, _, stage2_layer, _, _), scene, occluded, stats = out
        img = lambda t, c: t.reshape(height, width, c)
        mixed, share = occluded["mixed"], occluded["share"]
        passes = dict(color_scene=[img(t[0], 3) for t in scene], alpha_scene=[img(t[2], 1) for t in scene],
                      depth_scene=[img(t[1], 1) / far for t in scene],
                      color_occluded=img(mixed[0], 3), alpha_occluded=img(mixed[2], 1), depth_occluded=img(mixed[1], 1) / far,
                      color_scene_occluded=[img(t[0], 3) for t in occluded["scene"]],
                      alpha_scene_occluded=[img(t[2], 1) for t in occluded["scene"]],
                      depth_scene_occluded=[img(t[1], 1) / far for t in occluded["scene"]],
                      occluder_share=(img(share[0], 3), img(share[2], 1), img(share[1], 1) / far))
        return (img(mixed[0], 3), img(mixed[1], 1).clamp_min(0) / far, [img(t[0], 3) for t in stage2_layer],
                [img(t[1], 1) / far for t in stage2_layer], dict(stats, passes=passes))
    if accumulate is not None:
        from stnerf_amd.parallel import render_view_accumulated
        frame_ids = [0.0] * total_layers(model)
        for layer_id, frame_id in layer_frame_pair:
            frame_ids[layer_id] = float(frame_id)
        (stage2, _, stage2_layer, _, _), stats = render_view_accumulated(
            model, torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(pose, dtype=torch.float32), height, width, frame_ids,
            accumulate, density_threshold, bkgd_density_threshold, device=device, scene=bool(scene_passes), occluder=occluder,
            **(dict(lens=lens) if lens is not None else {}))
        stats = dict(stats, spp=stats["spp"].reshape(height, width), variance=stats["variance"].reshape(height, width, 3))
        return (stage2[0].reshape(height, width, 3), stage2[1].reshape(height, width, 1).clamp_min(0) / far,
                [t[0].reshape(height, width, 3) for t in stage2_layer], [t[1].reshape(height, width, 1) / far for t in stage2_layer],
                stats)
    occ_rows = None
    if occluder is not None:
        rgba, zbuf = (torch.as_tensor(x, dtype=torch.float32) for x in occluder)
        if tuple(rgba.shape) != (height, width, 4) or tuple(zbuf.shape) != (height, width):
            raise ValueError(f"render_pose: the occluder must be (rgba ({height},{width},4), depth ({height},{width})), got "
                             f"{tuple(rgba.shape)} and {tuple(zbuf.shape)}")
        occ_rows = torch.cat([rgba.reshape(-1, 4), zbuf.reshape(-1, 1).to(rgba.device)], 1).to(device).contiguous()
    frame_ids = [0.0] * total_layers(model)       # (the layer instances have their own frame ids)
    for layer_id, frame_id in layer_frame_pair:
        frame_ids[layer_id] = float(frame_id)
    out = render_view(model, torch.as_tensor(K, dtype=torch.float32), torch.as_tensor(pose, dtype=torch.float32), height, width,
                      frame_ids, density_threshold, bkgd_density_threshold, device=device, gather="fine",
                      **(dict(scene=True) if scene_passes else {}),
                      **(dict(occluder=occ_rows, occluder_stops=occluder_stops) if occ_rows is not None else {}),
                      **(dict(lens=lens) if lens is not None else {}), **(dict(deep=deep) if deep is not None else {}))
    occluded = frame = None
    if deep is not None:
        out, frame = out[:-1], out[-1]
        frame.far = float(far)
        if occ_rows is None:
            out = out if scene_passes else out[0]
    if occ_rows is not None:
        (stage2, _, stage2_layer, _, _), scene, occluded = out
    else:
        (stage2, _, stage2_layer, _, _), scene = out if scene_passes else (out, None)
    color = stage2[0].reshape(height, width, 3)
    depth = stage2[1].reshape(height, width, 1).clamp_min(0) / far
    color_layer = [t[0].reshape(height, width, 3) for t in stage2_layer]
    depth_layer = [t[1].reshape(height, width, 1) / far for t in stage2_layer]
    if not scene_passes and occluded is None:
        return (color, depth, color_layer, depth_layer) if frame is None else (color, depth, color_layer, depth_layer, dict(deep=frame))
    passes = dict(color_scene=[t[0].reshape(height, width, 3) for t in scene],
                  alpha_scene=[t[2].reshape(height, width, 1) for t in scene],
                  depth_scene=[t[1].reshape(height, width, 1) / far for t in scene])
    if occluded is not None:
        img = lambda t, c: t.reshape(height, width, c)
        mixed, share = occluded["mixed"], occluded["share"]
        passes.update(color_occluded=img(mixed[0], 3), alpha_occluded=img(mixed[2], 1), depth_occluded=img(mixed[1], 1) / far,
                      color_scene_occluded=[img(t[0], 3) for t in occluded["scene"]],
                      alpha_scene_occluded=[img(t[2], 1) for t in occluded["scene"]],
                      depth_scene_occluded=[img(t[1], 1) / far for t in occluded["scene"]],
                      occluder_share=(img(share[0], 3), img(share[2], 1), img(share[1], 1) / far))
    if frame is not None:
        passes["deep"] = frame
    return color, depth, color_layer, depth_layer, passes


def to_uint8(image: torch.Tensor) -> torch.Tensor:
    """[0,1] float image -> uint8 on the device (one small D2H afterwards instead of fp32 planes)."""
    return (image.clamp(0, 1) * 255.0 + 0.5).to(torch.uint8)
