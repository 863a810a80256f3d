#!/usr/bin/env python3
"""What deep frames cost and what they hold (GPU box): the bench's headline shape (taekwondo-1080p-64+64, split bf16, one GPU).
The scene is the SYNTHETIC FOG of ``bench.build_scene``: nearly every sample of every ray carries weight, so the samples per pixel
reported here are close to the worst case; on a real surface they will be far lower, and that is unmeasured.

1. Frames, alternating in one process after a warm-up: the scene passes alone and with ``deep=DeepSpec()``; the deep launches
   (count, offsets, fill) alone between device events, from the library's launch profiler.
2. Samples per pixel and bytes per frame for w_min in {0, 1e-4, 1e-3} x merge_dz in {0, one coarse step}.
3. ``DeepFrame.composite`` with E = 1 and E = 4 elements beside a re-render with ``occluder=``.
4. PSNR of the thresholded / merged frames' composites (E = 1, the disc of tools/bench_occluder.py) against the exact frame's.

    python tools/bench_deep.py --json deep.json
    python tools/bench_deep.py --record deep.json --bench-this a.json b.json c.json --bench-parent p.json q.json r.json \\
        --markdown profiles/deep_ab.md        # the tables from saved records and bench.py result lines (no GPU)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=2)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--reps", type=int, default=7, help="composite repetitions per leg")
ap.add_argument("--json", default=None, help="write the record here too")
ap.add_argument("--record", default=None, help="a saved record: measure nothing, only write the tables")
ap.add_argument("--bench-this", nargs="*", default=[], help="files with bench.py's JSON result line, this commit")
ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit, alternating with this commit's")
ap.add_argument("--markdown", default=None)
ap.add_argument("--note", default=None, help="a closing paragraph for the file")
args = ap.parse_args()
WORKLOAD = "taekwondo-1080p-64+64"


def spread(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def bench_line(path):
    """bench.py's one JSON result line out of a saved output."""
    for line in reversed(open(path).read().splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            return json.loads(line)
    raise ValueError(f"{path}: no JSON result line")


def write_markdown(rec, this, parent, path):
    med = statistics.median
    fr = rec["frames"]
    L = ["# Deep frames: what keeping the sample list costs, what it holds, and compositing on it", "",
         f"`tools/bench_deep.py`: {rec['workload']}, split bf16, one MI355X.  **The scene is the synthetic fog of `bench.build_scene`**: nearly "
         "every sample of every ray carries weight, so the samples per pixel below are close to the worst case l (n1 + n2) = "
         f"{rec['l'] * rec['S']}.  On a real surface they will be far lower; that is unmeasured.", "",
         "## Frames", "",
         f"{fr['warmup']} warm-up frame(s) per leg, then {fr['frames']} frames per leg (frame i from pose i), the legs alternating in one process; "
         "median (min .. max).  A deep frame renders in launch pieces of at most "
         f"{rec['piece_rays']:,} rays (the worst-case record buffer of a piece stays under 1 GiB) with one host sync per piece, the plain frame in "
         f"pieces of {rec['plain_piece_rays']:,}.", "",
         "| leg | s per frame | deep_count ms | deep_offsets ms | deep_fill ms |", "|---|---|---|---|---|"]
    for name, key in (("scene passes", "scene"), ("scene passes + deep", "deep")):
        d = fr[key]
        L.append(f"| {name} | {spread([x / 1e3 for x in d['frame_ms']])} | {med(d['deep_count_ms']):.3f} | {med(d['deep_offsets_ms']):.3f} | {med(d['deep_fill_ms']):.3f} |")
    L += ["", "The three deep columns are the frame's summed launches of that kernel between device events (the library's launch profiler).", "",
          "## What a frame holds", "", "| w_min | merge_dz | samples per pixel, mean | max | GB per frame |", "|---|---|---|---|---|"]
    for c in rec["configs"]:
        L.append(f"| {c['w_min']:g} | {c['merge_dz']:.4g} | {c['mean']:.1f} | {c['max']} | {c['bytes'] / 1e9:.2f} |")
    L += ["", f"merge_dz = one coarse step = {rec['coarse_step']:.4g}, measured on the exact frame: the median over the pixels of the depth span of "
          f"layer 0's records (last zf - first zf), over n1 = {rec['n1']}.", "",
          "## Compositing on the frame beside a re-render", "",
          f"`DeepFrame.composite` on the exact frame (w_min = 0, merge_dz = 0), {rec['reps']} repetitions, device events; the re-render is "
          "`render_view(occluder=)` of the same view, wall clock.", "",
          "| what | ms |", "|---|---|"]
    for name, key in (("flatten (E = 0)", "composite_0_ms"), ("composite, E = 1", "composite_1_ms"), ("composite, E = 4", "composite_4_ms"),
                      ("re-render with `occluder=`", "rerender_ms")):
        L.append(f"| {name} | {spread(rec[key])} |")
    L += ["", "## PSNR of an approximate frame's composite against the exact frame's (E = 1, the disc)", "",
          "| w_min | merge_dz | PSNR, dB |", "|---|---|---|"]
    for c in rec["configs"]:
        L.append(f"| {c['w_min']:g} | {c['merge_dz']:.4g} | {'exact' if c['psnr'] is None else format(c['psnr'], '.2f')} |")
    if this and parent:
        a, b = [bench_line(p)["value"] for p in this], [bench_line(p)["value"] for p in parent]
        unit = bench_line(this[0]).get("unit", "")
        L += ["", "## A render without the option against the parent commit", "",
              "`python bench.py --gpus 1 --steps 8 --warmup 3` from this tree and from a checkout of the parent commit with its own build of the "
              "library, alternating.", "", f"| run | this commit, {unit} | parent commit, {unit} |", "|---|---|---|"]
        L += [f"| {k + 1} | {x:,.0f} | {y:,.0f} |" for k, (x, y) in enumerate(zip(a, b))]
        L.append(f"| median (min .. max) | {med(a):,.0f} ({min(a):,.0f} .. {max(a):,.0f}) | {med(b):,.0f} ({min(b):,.0f} .. {max(b):,.0f}) |")
        sa, sb = (max(a) - min(a)) / med(a), (max(b) - min(b)) / med(b)
        L += ["", f"The medians differ by {100 * abs(med(a) - med(b)) / med(b):.3f} %; the spreads are {100 * sa:.3f} % (this commit) and {100 * sb:.3f} % "
              f"(parent): the bar is the larger, {100 * max(sa, sb):.3f} %."]
    if args.note:
        L += ["", args.note]
    with open(path, "w") as f:
        f.write("\n".join(L) + "\n")


if args.record:
    write_markdown(json.load(open(args.record)), args.bench_this, args.bench_parent, args.markdown)
    sys.exit(0)

sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from stnerf_amd import ops, synthetic as syn  # noqa: E402
from stnerf_amd.deep import DeepSpec, piece_rays  # noqa: E402
from stnerf_amd.parallel import render_view  # noqa: E402

model, (H, W, Lp, n1, n2, st, dt) = bench.build_scene(WORKLOAD, "cuda")
model.set_precision("bf16x3")
frame_ids = [1.0] + [2.5] * Lp
l, S = Lp + 1, n1 + n2


def frame(i, deep):
    K, T = syn.camera(H, W, orbit_deg=10.0 + 1.5 * i)
    model.seed = i
    torch.cuda.synchronize()
    ops.profile_begin()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = render_view(model, K, T, H, W, frame_ids, **(dict(deep=deep) if deep is not None else dict(scene=True)))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    per = {}
    for r in ops.profile_end():
        per[r["kernel"]] = per.get(r["kernel"], 0.0) + r["ms"]
    return ms, per, out


runs = dict(scene=[], deep=[])
for i in range(-args.warmup, args.frames):
    for leg in ("scene", "deep"):
        ms, per, out = frame(i, DeepSpec() if leg == "deep" else None)
        del out
        torch.cuda.empty_cache()
        if i >= 0:
            runs[leg].append((ms, per))
digest = lambda rows: dict(frame_ms=[round(r[0], 2) for r in rows], **{k + "_ms": [round(r[1].get(k, 0.0), 4) for r in rows]
                                                                       for k in ("deep_count", "deep_offsets", "deep_fill")})
frames = {k: digest(v) for k, v in runs.items()}
frames.update(frames=args.frames, warmup=args.warmup)

# ---- the exact frame, and from it the depth scale: one coarse step = the median span of layer 0's records over n1
_, _, out0 = frame(0, DeepSpec())
exact = out0[-1]
del out0
layer0 = (exact.meta()[0] == 0)
zf = exact.samples[:, 5]
pixel = torch.repeat_interleave(torch.arange(H * W, device=zf.device), exact.offsets[1:] - exact.offsets[:-1])[layer0]
lo = torch.full((H * W,), float("inf"), device=zf.device).scatter_reduce(0, pixel, zf[layer0], "amin")
hi = torch.full((H * W,), float("-inf"), device=zf.device).scatter_reduce(0, pixel, zf[layer0], "amax")
seen = torch.isfinite(lo) & torch.isfinite(hi)
coarse_step = float((hi - lo)[seen].median()) / n1
z_mid = float((0.5 * (hi + lo))[seen].median())

# ---- the element: tools/bench_occluder.py's disc, at the middle of that span
y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
r = torch.sqrt((y - (H - 1) / 2) ** 2 + (x - (W - 1) / 2) ** 2)
disc = torch.zeros(H * W, 5, device="cuda")
disc[:, 0], disc[:, 1], disc[:, 2] = 0.9, 0.6, 0.1
disc[:, 3] = torch.where(r <= H / 12, 1.0, torch.where(r <= H / 6, 0.5, 0.0)).reshape(-1)
disc[:, 4] = z_mid
del layer0, zf, pixel, lo, hi, seen


def event_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


configs, exact_image, rec_extra = [], None, {}
for w_min in (0.0, 1e-4, 1e-3):
    for dz in (0.0, coarse_step):
        if exact is not None:
            fr, exact = exact, None
        else:
            _, _, out = frame(0, DeepSpec(w_min, dz))
            fr = out[-1]
            del out
        stats = fr.stats()
        mixed = fr.composite(disc[:, None, :].contiguous(), want_scene=False, want_shares=False)[0][:, 0:3]
        torch.cuda.synchronize()
        if exact_image is None:
            exact_image = mixed.clone()
            four = torch.stack([disc, disc, disc, disc], 1).contiguous()
            four[:, :, 4] += torch.arange(4, device="cuda") * coarse_step
            for name, el in (("composite_0_ms", None), ("composite_1_ms", disc[:, None, :].contiguous()), ("composite_4_ms", four)):
                rec_extra[name] = [event_ms(lambda: fr.composite(el)) for _ in range(args.reps + 2)][2:]
            psnr = None
        else:
            mse = float(((mixed - exact_image) ** 2).mean())
            psnr = None if mse == 0 else -10.0 * math.log10(mse)
        configs.append(dict(w_min=w_min, merge_dz=dz, mean=stats["mean"], max=stats["max"], bytes=stats["bytes"], psnr=psnr))
        del fr, mixed
        torch.cuda.empty_cache()

rerender = []
K0, T0 = syn.camera(H, W, orbit_deg=10.0)
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = render_view(model, K0, T0, H, W, frame_ids, occluder=disc)
    torch.cuda.synchronize()
    rerender.append((time.perf_counter() - t0) * 1e3)
    del out

rec = dict(workload=WORKLOAD, precision="bf16x3", l=l, S=S, n1=n1, piece_rays=min(piece_rays(l, S), int(model.max_rays_per_launch)),
           plain_piece_rays=int(model.max_rays_per_launch), coarse_step=coarse_step, z_element=z_mid, frames=frames, configs=configs,
           reps=args.reps, rerender_ms=rerender, **rec_extra)
print(json.dumps(rec))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rec, f)
if args.markdown:
    write_markdown(rec, args.bench_this, args.bench_parent, args.markdown)
