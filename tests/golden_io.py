"""Reading the fixtures of tests/golden/make_golden.py --real-counts, which differ from the older ones in two respects:

* a fixture too large for one committed file is split over ``name.npz``, ``name.part2.npz``, ... (``meta["parts"]``);
* the uniform draws are stored as seeds and shapes (``meta["draw_seed_base"]`` / ``meta["draw_shapes"]``, as train_tf_trainer's
  are): draw k = torch.rand(shape, generator=manual_seed(base + k)) on the CPU.  A teacher-forced fixture's ``u{i}`` are draws too.

``load_golden`` here returns every fixture, old or new, with the keys the older ones have."""
import os

import numpy as np
import torch

import conftest


def load_golden(name):
    """-> (meta dict, {key: torch tensor}), parts merged and seeded draws regenerated as ``draw{i}`` (and ``u{i}``)."""
    meta, arrs = conftest.load_golden(name)
    for g in range(2, meta.get("parts", 1) + 1):
        z = np.load(os.path.join(conftest.GOLDEN, f"{name}.part{g}.npz"))
        assert not set(z.files) & set(arrs), (name, g)
        arrs.update({k: torch.from_numpy(z[k]) for k in z.files})
    if "draw_seed_base" in meta:
        assert len(meta["draw_shapes"]) == meta["n_draws"]
        for k, shape in enumerate(meta["draw_shapes"]):
            arrs[f"draw{k}"] = torch.rand(tuple(shape), generator=torch.Generator().manual_seed(meta["draw_seed_base"] + k))
        if "pdf_t0" in arrs:                       # teacher-forced: one call, l jitter draws then l resampling draws
            l = meta["L"] + 1
            for i in range(l):
                arrs[f"u{i}"] = arrs[f"draw{l + i}"]
    return meta, arrs


def load_ray_views():
    """generate_rays_views -> {tag: dict(K, T, h, w, rays (n, 6), pixels (n,) int32 or None)}: "a" a whole 270 x 480 view, "b" a
    sorted list of 32,768 pixels of a 1080p view; the rows are the reference's generate_rays rows of those pixels."""
    meta, a = load_golden("generate_rays_views")
    views = {}
    for tag in ("a", "b"):
        dirs = torch.cat([a[f"dirs_{tag}{b}"] for b in range(meta[f"blocks_{tag}"])], 0)
        T = a[f"T_{tag}"]
        rays = torch.cat([T[:3, 3].expand(dirs.shape[0], 3), dirs], 1).contiguous()
        views[tag] = dict(K=a[f"K_{tag}"], T=T, h=meta[f"h_{tag}"], w=meta[f"w_{tag}"], rays=rays, pixels=a.get(f"pixels_{tag}"),
                          norms_differ=meta[f"norms_differ_{tag}"])
    assert views["a"]["rays"].shape[0] == views["a"]["h"] * views["a"]["w"] and views["a"]["pixels"] is None
    assert views["b"]["rays"].shape[0] == views["b"]["pixels"].shape[0]
    return views
