#!/usr/bin/env python3
"""What depth-tested occluder compositing costs and what its stop saves (GPU box): the bench's headline shape
(taekwondo-1080p-64+64, split bf16, one GPU) with a synthetic occluder -- a disc over the central third of the image at a ray
parameter in front of the performers, a = 1 inside a disc of half the radius and a = 0.5 in the ring around it.

1. The new launch beside ``layer_scene_kernel`` on the SAME buffers, at op level on one launch piece of the frame (2^19 rays x l x
   (n1 + n2) samples, every layer live on every ray): stnerf_composite_scene with the merged weights alone and with the scene pass
   (the difference is ``layer_scene_kernel``, which moves the same 24 B per sample), then stnerf_scene_occluder with every row
   present and with the disc's rows; alternating, medians and spreads, and the launch's bytes over the box's copy rate
   (profiles/r03_hbm_copy_microbench.json).
2. Frames, alternating in one process after a warm-up: the scene passes alone, with the occluder, with early ray termination
   attached and the occluder stop off and on (rows listed per layer from ``Termination.stats()``).

    python tools/bench_occluder.py --json occluder.json
    python tools/bench_occluder.py --record occluder.json --bench-this a.json b.json c.json --bench-parent p.json q.json r.json \\
        --markdown profiles/occluder_ab.md        # the tables from saved records and bench.py result lines (no GPU)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--reps", type=int, default=7, help="op-level repetitions per leg")
ap.add_argument("--json", default=None, help="write the record here too")
ap.add_argument("--record", default=None, help="a saved record: measure nothing, only write the tables")
ap.add_argument("--bench-this", nargs="*", default=[], help="files with bench.py's JSON result line, this commit")
ap.add_argument("--bench-parent", nargs="*", default=[], help="the same of the parent commit, alternating with this commit's")
ap.add_argument("--markdown", default=None)
ap.add_argument("--note", default=None, help="a closing paragraph for the file")
args = ap.parse_args()
WORKLOAD = "taekwondo-1080p-64+64"
COPY_GBPS = json.load(open(os.path.join(ROOT, "profiles", "r03_hbm_copy_microbench.json")))["copy_GBps"]


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
    op, fr = rec["op_level"], rec["frames"]
    med = statistics.median
    scene_ms = med(op["layer_scene_ms"])
    L = ["# Depth-tested occluder compositing: the new launch, the occluder stop, and a render without an occluder", "",
         f"`tools/bench_occluder.py`: {rec['workload']}, split bf16, one MI355X.  Occluder: a disc over the central third of the image "
         f"(radius H / 6 = {rec['occluder']['radius']} px, {rec['occluder']['present_rays']:,} of {rec['occluder']['rays']:,} rays present) at ray "
         f"parameter z = {rec['occluder']['z']:.3f}, in front of the performers (their nearest composited depth under the disc: "
         f"{rec['occluder']['nearest_performer_depth']:.3f}); a = 1 inside half the radius ({rec['occluder']['opaque_rays']:,} rays), a = 0.5 in the ring.", "",
         "## The new launch beside `layer_scene_kernel`, same buffers", "",
         f"One launch piece of the frame at op level: n = {op['n']:,} rays, l = {op['l']}, S = {op['S']}, every layer live on every ray; "
         f"{op['reps']} repetitions per leg, the legs alternating, HIP events of the library's launch profiler; median (min .. max) in ms.  "
         "`layer_scene_kernel` is the difference, repetition by repetition, of `stnerf_composite_scene` with and without the scene pass (its "
         "other launches are the same).  Bytes: 24 B per sample read on a present ray (t, merged weight, raw float4), 20 B per layer and "
         "output written; an absent ray moves its rows only.", "",
         "| launch | ms | GB moved | GB/s | of the copy rate |", "|---|---|---|---|---|"]
    for name, ms, gb in (("`layer_scene_kernel` (by difference)", op["layer_scene_ms"], op["scene_gb"]),
                         ("`scene_occluder_kernel`, every row present", op["occluder_all_ms"], op["occluder_all_gb"]),
                         ("`scene_occluder_kernel`, every row present, all five outputs", op["occluder_all5_ms"], op["occluder_all5_gb"]),
                         ("`scene_occluder_kernel`, the disc's rows", op["occluder_disc_ms"], op["occluder_disc_gb"])):
        rate = gb / (med(ms) * 1e-3)
        L.append(f"| {name} | {spread(ms)} | {gb:.3f} | {rate:.0f} | {rate / COPY_GBPS:.2f} |")
    L += ["", f"Copy rate of the box: {COPY_GBPS} GB/s (`profiles/r03_hbm_copy_microbench.json`, float4 copy).  The margin of the comparison is the "
          f"session's run-to-run spread: `layer_scene_kernel` {min(op['layer_scene_ms']):.3f} .. {max(op['layer_scene_ms']):.3f} ms, the new launch "
          f"{min(op['occluder_all_ms']):.3f} .. {max(op['occluder_all_ms']):.3f} ms; ratio of the medians {med(op['occluder_all_ms']) / scene_ms:.3f}.", "",
          "## Frames", "",
          f"{fr['warmup']} warm-up frame(s) per leg, then {fr['frames']} frames per leg (frame i from pose i), the legs alternating in one process; "
          "ms per frame, median (min .. max).  `scene_occluder` / `occluder_stop`: the frame's summed launches of that kernel.", "",
          "| leg | frame ms | scene_occluder ms | occluder_stop ms |", "|---|---|---|---|"]
    for name, key in (("scene passes, no occluder", "scene"), ("occluder", "occluded"), ("termination, occluder, stop off", "term_off"),
                      ("termination, occluder, stop on", "term_on")):
        d = fr[key]
        L.append(f"| {name} | {spread(d['frame_ms'])} | {med(d['scene_occluder_ms']):.3f} | {med(d['occluder_stop_ms']):.3f} |")
    L += ["", "Rows listed by the terminated layers' row lists per frame (fine samples that reach a network), stop off -> on:", "",
          "| layer | tested | listed, stop off | listed, stop on | saved |", "|---|---|---|---|---|"]
    for i in sorted(fr["rows_off"], key=int):
        t, s0 = fr["rows_off"][i]
        _, s1 = fr["rows_on"][i]
        L.append(f"| {i} | {t:,} | {t - s0:,} | {t - s1:,} | {s1 - s0:,} ({100.0 * (s1 - s0) / max(t - s0, 1):.2f} %) |")
    if this and parent:
        a, b = [bench_line(p)["value"] for p in this], [bench_line(p)["value"] for p in parent]
        unit = bench_line(this[0]).get("unit", "")
        L += ["", "## A render without an occluder against the parent commit", "",
              f"`python bench.py --gpus 1 --steps {rec.get('bench_steps', 5)} --warmup {rec.get('bench_warmup', 2)}` from this tree and from a checkout of the "
              "parent commit with its own build of the library, alternating, three times each in one GPU visit.", "",
              f"| run | this commit, {unit} | parent commit, {unit} |", "|---|---|---|"]
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
from stnerf_amd import hip, ops, synthetic as syn  # noqa: E402
from stnerf_amd.parallel import render_view  # noqa: E402

model, (H, W, L, n1, n2, st, dt) = bench.build_scene(WORKLOAD, "cuda")
model.set_precision("bf16x3")
frame_ids = [1.0] + [2.5] * L
l, S = L + 1, n1 + n2


def disc(z):
    """The occluder's rows (H W, 5) on the device: colour (0.9, 0.6, 0.1), a = 1 within H / 12 of the image centre, 0.5 out to H / 6."""
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    r = torch.sqrt((y - (H - 1) / 2) ** 2 + (x - (W - 1) / 2) ** 2)
    a = torch.where(r <= H / 12, 1.0, torch.where(r <= H / 6, 0.5, 0.0))
    occ = torch.zeros(H * W, 5, device="cuda")
    occ[:, 0], occ[:, 1], occ[:, 2], occ[:, 3], occ[:, 4] = 0.9, 0.6, 0.1, a.reshape(-1), z
    return occ


# ---- where the performers are: the nearest composited performer depth under the disc in an unoccluded frame
K0, T0 = syn.camera(H, W, orbit_deg=10.0)
with torch.no_grad():
    (_, _, fine_layer, _, _), _ = render_view(model, K0, T0, H, W, frame_ids, scene=True)
under = disc(0.0)[:, 3] > 0
nearest = min(float((d[under] / a[under])[a[under, 0] > 0.05].min()) for _, d, a in fine_layer[1:] if bool((a[under, 0] > 0.05).any()))
Z = 0.8 * nearest
OCC = disc(Z)
occluder_info = dict(radius=H // 6, rays=H * W, present_rays=int((OCC[:, 3] > 0).sum()), opaque_rays=int((OCC[:, 3] >= 1).sum()), z=Z,
                     nearest_performer_depth=nearest)
del fine_layer
torch.cuda.empty_cache()


# ---- 1. op level: one launch piece
def op_level():
    n = 1 << 19
    g = torch.Generator(device="cuda").manual_seed(1)
    t = (2.0 + torch.cumsum(torch.rand(n, l, S, device="cuda", generator=g) * 0.05 + 0.001, -1)).contiguous()
    raw = torch.randn(n, l, S, 4, device="cuda", generator=g)
    raw[..., 3] = raw[..., 3].abs() * 0.5
    mask = torch.ones(n, l, dtype=torch.uint8, device="cuda")
    p = ops.composite_params(fine=True, evaluated=[2] + [1] * L, rgb_activated=True)
    new = lambda *s: torch.empty(*s, device="cuda")
    layer_out, mixed, merged, scene, scratch = new(n, l, 5), new(n, 5), new(n, l, S), new(n, l, 5), torch.empty(n, dtype=torch.uint8, device="cuda")
    outs = [new(n, 5), new(n, l, 5), new(n, 5), new(n, l, 5), new(n, l, 5)]
    rows_all = OCC[OCC[:, 3] > 0][:1].expand(n, 5).contiguous()                   # every row present (the ring's row)
    rows_all[:, 4] = t[:, 0, S // 2]                                              # ... at a depth inside the ray
    rows_disc = OCC[torch.randperm(H * W, device="cuda", generator=g)[:n]].contiguous()               # the disc's share of present rows
    rows_disc[:, 4] = torch.where(rows_disc[:, 3] > 0, t[:, 0, S // 2], rows_disc[:, 4])
    null = C.c_void_p(0)

    def timed(call):
        torch.cuda.synchronize()
        ops.profile_begin()
        call()
        torch.cuda.synchronize()
        return sum(r["ms"] for r in ops.profile_end())

    def composite(with_scene):
        hip.check(hip.lib().stnerf_composite_scene(hip.dptr(t), hip.dptr(raw), hip.dptr(mask, torch.uint8), n, l, S, C.byref(p), hip.dptr(layer_out),
                                                   hip.dptr(mixed), null, null, hip.dptr(scratch, torch.uint8), hip.dptr(merged),
                                                   hip.dptr(scene) if with_scene else null, hip.stream_ptr()), "stnerf_composite_scene")

    def occluder(rows, k):
        hip.check(hip.lib().stnerf_scene_occluder(hip.dptr(t), hip.dptr(raw), hip.dptr(mask, torch.uint8), hip.dptr(merged), n, l, S, C.byref(p),
                                                  hip.dptr(scene), hip.dptr(mixed), hip.dptr(rows), *[hip.dptr(o) if j < k else null for j, o in enumerate(outs)],
                                                  hip.stream_ptr()), "stnerf_scene_occluder")
    legs = dict(a=[], b=[], all=[], all5=[], disc=[])
    for rep in range(-2, args.reps):                       # two warm-up rounds
        row = dict(a=timed(lambda: composite(False)), b=timed(lambda: composite(True)), all=timed(lambda: occluder(rows_all, 3)),
                   all5=timed(lambda: occluder(rows_all, 5)), disc=timed(lambda: occluder(rows_disc, 3)))
        if rep >= 0:
            for k, v in row.items():
                legs[k].append(v)
    present = int((rows_disc[:, 3] > 0).sum())
    sample_gb = lambda rays: rays * (24.0 * l * S + l) / 1e9
    return dict(n=n, l=l, S=S, reps=args.reps, composite_ms=legs["a"], composite_scene_ms=legs["b"],
                layer_scene_ms=[b - a for a, b in zip(legs["a"], legs["b"])], scene_gb=sample_gb(n) + n * 20.0 * l / 1e9,
                occluder_all_ms=legs["all"], occluder_all_gb=sample_gb(n) + n * 20.0 * (1 + 2 + l) / 1e9,
                occluder_all5_ms=legs["all5"], occluder_all5_gb=sample_gb(n) + n * 20.0 * (1 + 2 + 3 * l) / 1e9,
                occluder_disc_ms=legs["disc"], disc_present_rays=present,
                occluder_disc_gb=sample_gb(present) + n * 20.0 * (1 + 2 + l) / 1e9 + (n - present) * 20.0 * (1 + l) / 1e9)


op = op_level()
torch.cuda.empty_cache()


# ---- 2. frames
def frame(i, leg):
    K, T = syn.camera(H, W, orbit_deg=10.0 + 1.5 * i)
    model.seed = i
    model.set_termination(1e-4 if leg.startswith("term") else None)
    kw = dict(scene=True) if leg == "scene" else dict(occluder=OCC, occluder_stops=leg == "term_on")
    if model.termination is not None:
        model.termination.reset_stats()
    torch.cuda.synchronize()
    ops.profile_begin()
    t0 = time.perf_counter()
    with torch.no_grad():
        render_view(model, K, T, H, W, frame_ids, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    per = {}
    for r in ops.profile_end():
        per[r["kernel"]] = per.get(r["kernel"], 0.0) + r["ms"]
    rows = model.termination.stats()["rows"] if model.termination is not None else None
    return ms, per, rows


LEGS = ("scene", "occluded", "term_off", "term_on")
runs = {k: [] for k in LEGS}
for i in range(-args.warmup, args.frames):
    for leg in LEGS:
        out = frame(i, leg)
        if i >= 0:
            runs[leg].append(out)
model.set_termination(None)
digest = lambda rows: dict(frame_ms=[round(r[0], 2) for r in rows], scene_occluder_ms=[round(r[1].get("scene_occluder", 0.0), 4) for r in rows],
                           occluder_stop_ms=[round(r[1].get("occluder_stop", 0.0), 4) for r in rows],
                           composite_ms=[round(r[1].get("composite", 0.0), 3) for r in rows], mlp_stage_ms=[round(r[1].get("mlp_stage", 0.0), 2) for r in rows])
frames = {k: digest(v) for k, v in runs.items()}
frames.update(frames=args.frames, warmup=args.warmup, rows_off={str(i): list(v) for i, v in runs["term_off"][-1][2].items()},
              rows_on={str(i): list(v) for i, v in runs["term_on"][-1][2].items()})
rec = dict(workload=WORKLOAD, precision="bf16x3", occluder=occluder_info, op_level=op, frames=frames)
print(json.dumps(rec))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rec, f)
if args.markdown:
    write_markdown(rec, args.bench_this, args.bench_parent, args.markdown)
