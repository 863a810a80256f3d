"""Reprojection of the background across nearby views: host logic, built only from calls that exist --
``ops.reproject`` (csrc/reproject.hip), ``ops.generate_rays(pixels=)``, ``render_rays_raw`` and ``render_rays_occluded``.

A key view's layer 0, rendered alone, is a ``BackgroundPlate``: straight colour, alpha and the expected ray parameter per pixel.
Warped into a neighbouring view it covers almost every pixel; the pixels it cannot cover are rendered (layer 0 only) and
scattered into the warped rows; the finished plate is then an occluder row per ray, composited into the scene with
``display_layers[0] = 0``.  That flag does NOT skip layer 0's networks inside the render call (the pipeline evaluates the background
on every ray of every call and never reads its shown flag), so such a frame pays for the whole background again and composites it
beside the plate.  ``ReprojectSpec(exclusive=True)`` is the mode that saves the work: no hole is rendered separately, and ONE
``render_rays_occluded(background_rays=)`` call evaluates layer 0 exactly on the rays whose plate row is absent (the per-ray
background mask, include/stnerf.h) -- one source of background per ray.  Approximate by nature (one depth per pixel, the view
dependence frozen at the key view): opt-in, inference only, one rank."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch

# The defaults are read off the sweep of profiles/reproject_ab.md (PSNR against hole fraction): the widest guard and the highest
# alpha floor of the sweep -- the fewest holes at no loss, and the best PSNR at every guard.
DEFAULT_REL = 0.2
DEFAULT_A_MIN = 0.9


class ReprojectSpec:
    """``key_every`` = N >= 1: key plates at path indices 0, N, 2N, ...; ``rel`` >= 0: the resolve guard (a warped pixel whose ray
    parameter exceeds the nearest of its 3x3 neighbourhood by more than the factor 1 + rel is rendered instead); ``a_min`` in
    [0, 1]: a plate row whose alpha is below it carries no depth and is absent.  ``exclusive`` (False: the frames as they always
    were): the background comes from exactly one source per ray -- the plate where its row is present, the networks where it is
    absent, in one render call under a per-ray background mask; no hole is rendered separately."""

    def __init__(self, key_every: int = 4, rel: float = DEFAULT_REL, a_min: float = DEFAULT_A_MIN, exclusive: bool = False):
        if isinstance(key_every, bool) or not isinstance(key_every, int) or key_every < 1:
            raise ValueError(f"ReprojectSpec: key_every is a whole number >= 1, got {key_every!r}")
        rel, a_min = float(rel), float(a_min)
        if not (rel >= 0.0) or math.isinf(rel):
            raise ValueError(f"ReprojectSpec: rel must be finite and >= 0, got {rel!r}")
        if not (0.0 <= a_min <= 1.0):
            raise ValueError(f"ReprojectSpec: a_min must lie in [0, 1], got {a_min!r}")
        if not isinstance(exclusive, bool):
            raise ValueError(f"ReprojectSpec: exclusive is True or False, got {exclusive!r}")
        self.key_every, self.rel, self.a_min, self.exclusive = key_every, rel, a_min, exclusive

    def __repr__(self):
        return (f"ReprojectSpec(key_every={self.key_every}, rel={self.rel}, a_min={self.a_min}"
                + (", exclusive=True)" if self.exclusive else ")"))

    def keys_of(self, i: int, n_poses: int) -> Tuple[int, ...]:
        """The key indices frame ``i`` of a path of ``n_poses`` may use: floor(i / N) N, and that plus N where the path has it."""
        if not 0 <= i < n_poses:
            raise ValueError(f"ReprojectSpec.keys_of: frame {i} outside a path of {n_poses} poses")
        k0 = i // self.key_every * self.key_every
        return (k0, k0 + self.key_every) if k0 + self.key_every < n_poses else (k0,)


def as_spec(spec) -> ReprojectSpec:
    """A ``ReprojectSpec`` from one or from the dict of its arguments."""
    if isinstance(spec, ReprojectSpec):
        return spec
    if isinstance(spec, dict):
        return ReprojectSpec(**spec)
    raise TypeError(f"reproject is a ReprojectSpec or the dict of its arguments, got {type(spec).__name__}")


def absent_rows(rows: torch.Tensor) -> torch.Tensor:
    """(n,) bool: the occluder's own rule for an ABSENT row {r, g, b, a, z} (include/stnerf.h): a <= 0 or NaN, or z not finite."""
    return ~(rows[:, 3] > 0) | ~torch.isfinite(rows[:, 4])


def plate_rows(mixed: torch.Tensor, a_min: float) -> torch.Tensor:
    """(n,5) {premultiplied r, g, b, weighted depth, alpha} of layer 0 composited alone -> (n,5) plate rows {r/a, g/a, b/a, a,
    depth/a}: straight colour, alpha, expected ray parameter -- an occluder row.  A row with a < a_min (or NaN) is absent: zeros
    and a NaN depth.  THE function that makes a key's rows and a hole's."""
    a = mixed[:, 4:5]
    rows = torch.cat([mixed[:, 0:3] / a, a, mixed[:, 3:4] / a], 1)
    absent = torch.zeros(5, dtype=mixed.dtype, device=mixed.device)
    absent[4] = float("nan")
    return torch.where(a >= a_min, rows, absent).contiguous()


def view_thresholds(h: int, w: int, chuncks: int, density_threshold, bkgd_density_threshold):
    """The thresholds a view of h w rays renders with (``layered_batchify_ray``'s rule: a view of less than one chunk takes the
    model's defaults) -> the keywords of ``render_rays_raw`` / ``render_rays_occluded``."""
    if h * w < chuncks:
        return {}
    return dict(only_coarse=False, density_threshold=density_threshold, bkgd_density_threshold=bkgd_density_threshold, ref_chunk=chuncks)


def background_identity(model, frame_ids, h: int, w: int, chuncks: int, density_threshold, bkgd_density_threshold):
    """What layer 0's plate rows depend on besides the camera, as a hashable host value: the background cache's group key
    (``LayeredRFRender.background_cache_key``: seed, sample counts, arithmetic, ray format, edited box, layer 0's point un-edit
    and rotation, near and border, model flags, parameter versions, an attached background grid's identity and -- only where
    the background is time-dependent -- layer 0's frame id) with an empty view, plus what acts after the networks: layer 0's
    opacity entry, alpha, and the thresholds the view renders with."""
    retiming = len(frame_ids) == model.total_layers and model.total_layers > 1
    group, _ = model.background_cache_key(((), float(frame_ids[0])), (0, 0), (0, 0, 0), retiming, False)
    table = model._layer_alpha_table()
    kw = view_thresholds(h, w, chuncks, density_threshold, bkgd_density_threshold)
    thr = (float(kw["density_threshold"]), float(kw["bkgd_density_threshold"])) if kw else None
    return group, None if table is None else float(table[0]), float(model.alpha), thr


def refuse(model, what: str) -> None:
    """The refusals every entry of this module shares: more than one rank, training mode, a hidden background."""
    from stnerf_amd import parallel
    if parallel.active_group(model) is not None:
        raise RuntimeError(f"{what} under shard_views with more than one rank: the plates live on one device and multi-rank "
                           "reprojection is out of scope; render on one rank (model.shard_views = False)")
    if torch.is_grad_enabled() and model.training and any(p.requires_grad for p in model.parameters()):
        raise RuntimeError(f"{what} in training mode: reprojection is inference only (that call would take the op-by-op path, which "
                           "has no occluder composite); call model.eval() or wrap the render in torch.no_grad()")
    if not model.is_shown_layer(0):
        raise ValueError(f"{what} with layer 0 hidden: there is no background to reproject")


def render_background_only(model, rays: torch.Tensor, kw: dict) -> torch.Tensor:
    """Layer 0's own (n,5) {r, g, b, depth, alpha} of ``rays`` -- the per-layer output, layer 0 composited alone -- with every layer
    but 0 hidden, which skips their networks; ``display_layers``, the view key and the seed restored in a ``finally``.  Not the
    mixed output: a hidden layer's samples still cut the intervals of the merged list, so the mixed image of layer 0 alone
    follows the performers' boxes, and with them their frame ids; the per-layer one does not.  No cache serves the call (the rays
    may be a pixel list)."""
    saved = dict(model.display_layers)
    saved_key, saved_ids, saved_seed = getattr(model, "view_key", None), getattr(model, "view_frame_ids", None), model.seed
    try:
        for i in saved:
            model.display_layers[i] = 1 if i == 0 else 0
        model.view_key, model.view_frame_ids = None, None
        with torch.no_grad():
            return model.render_rays_raw(rays, **kw)[2][:, 0].contiguous()
    finally:
        model.display_layers.clear()
        model.display_layers.update(saved)
        model.view_key, model.view_frame_ids, model.seed = saved_key, saved_ids, saved_seed


class BackgroundPlate:
    """A key view's layer 0 alone: the camera ``(K, T, h, w)``, ``rows`` (h w, 5) = {r/a, g/a, b/a, a, depth/a}, ``t`` = the
    depth column (NaN: absent), and ``identity`` = what layer 0 depended on besides the camera (``background_identity``).
    ``index``: the plate's place on a path, or None."""

    def __init__(self, K, T, h: int, w: int, rows: torch.Tensor, identity, index: Optional[int] = None):
        if rows.dim() != 2 or tuple(rows.shape) != (h * w, 5):
            raise ValueError(f"BackgroundPlate: rows must be ({h * w}, 5), got {tuple(rows.shape)}")
        self.K = torch.as_tensor(K, dtype=torch.float32).detach().cpu().clone()
        self.T = torch.as_tensor(T, dtype=torch.float32).detach().cpu().clone()
        self.h, self.w, self.rows, self.identity, self.index = int(h), int(w), rows, identity, index
        self.t = rows[:, 4].contiguous()

    def source(self):
        """The plate as a source of ``ops.reproject``."""
        return self.K, self.T, self.h, self.w, self.rows, self.t

    @classmethod
    def render(cls, model, K, T, h: int, w: int, frame_ids, spec, density_threshold=0.0, bkgd_density_threshold=0.0,
               chuncks: int = 512 * 7, device="cuda", index: Optional[int] = None) -> "BackgroundPlate":
        """Render the view with every layer but 0 hidden (``render_rays_raw``) and keep it as a plate."""
        from stnerf_amd import ops
        spec = as_spec(spec)
        refuse(model, "BackgroundPlate.render")
        frame_ids = [float(f) for f in frame_ids]
        identity = background_identity(model, frame_ids, h, w, chuncks, density_threshold, bkgd_density_threshold)
        rays = ops.generate_rays(K, T, h, w, frame_ids=frame_ids, device=device)
        mixed = render_background_only(model, rays, view_thresholds(h, w, chuncks, density_threshold, bkgd_density_threshold))
        return cls(K, T, h, w, plate_rows(mixed, spec.a_min), identity, index)


def warp_plates(model, K, T, h: int, w: int, frame_ids, plates: Sequence[BackgroundPlate], spec, density_threshold=0.0,
                bkgd_density_threshold=0.0, chuncks: int = 512 * 7, device="cuda", render_holes: bool = True):
    """Steps 1 and 2 of ``parallel.render_view_reprojected``: the plates' rows warped into the view, its holes rendered (layer 0
    only) and scattered in -> (rows (h w, 5) occluder rows, holes (n_holes,) int32, n_holes, warped) with ``warped`` =
    ``ops.reproject``'s (values, t, src) -- or None where a plate of this very camera was taken as it is (no launch).
    ``render_holes=False`` stops after the warp: no ray is generated or rendered, and a hole's row stays absent (zeros, a NaN
    depth) -- what the exclusive mode hands to the per-ray background mask."""
    from stnerf_amd import ops
    spec = as_spec(spec)
    if not plates:
        raise ValueError("reproject: no plate given")
    frame_ids = [float(f) for f in frame_ids]
    identity = background_identity(model, frame_ids, h, w, chuncks, density_threshold, bkgd_density_threshold)
    for p in plates:
        if p.identity != identity:
            raise ValueError("reproject: a plate was rendered under another background (layer 0's frame id, edit, opacity, "
                             "thresholds, precision, seed, weights or grid differ from this frame's); render a new key plate")
    Kf, Tf = torch.as_tensor(K, dtype=torch.float32).detach().cpu(), torch.as_tensor(T, dtype=torch.float32).detach().cpu()
    for p in plates:
        # a plate of THIS camera (the same K, T, h, w, bit for bit): the warp is the identity by definition, so its rows are the
        # frame's as they are -- through the kernels its depths would come back one rounding away (t' = |t d|, |d| = 1 +- an ulp)
        if (p.h, p.w) == (h, w) and torch.equal(p.K, Kf) and torch.equal(p.T, Tf):
            return p.rows.clone(), torch.empty(0, dtype=torch.int32, device=p.rows.device), 0, None
    values, t, src, holes, n_holes = ops.reproject([p.source() for p in plates], K, T, h, w, spec.rel)
    rows = values.clone()
    rows[:, 4] = t                       # the ray parameter in THIS view (a hole: NaN, absent until it is rendered)
    if n_holes and render_holes:
        rays = ops.generate_rays(K, T, h, w, frame_ids=frame_ids, device=device, pixels=holes)
        mixed = render_background_only(model, rays, view_thresholds(h, w, chuncks, density_threshold, bkgd_density_threshold))
        rows[holes.long()] = plate_rows(mixed, spec.a_min)
    return rows, holes, n_holes, (values, t, src)
