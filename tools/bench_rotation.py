#!/usr/bin/env python3
"""What a per-layer rotation costs (GPU box): the bench's headline shape (taekwondo-1080p-64+64, split bf16, one GPU), unrotated
and one-performer-rotated frames ALTERNATING in one process, three each after the warm-up, every frame under the library's launch
profiler (ops.profile_begin / profile_end).  Reports per leg the frame times and the summed sampler / resampler kernel times of a
frame; the ray-bias launches have no profiler record of their own (the stage's record covers them), so the ray-bias kernel is
timed at op level on one launch piece, plain and rotated.

    python tools/bench_rotation.py                                  # both legs of this checkout -> JSON on stdout
    python tools/bench_rotation.py --tree DIR --legs plain --json a.json    # the unrotated leg of ANOTHER checkout (built in place),
                                                                            # e.g. the parent commit, run twice for its own spread
    python tools/bench_rotation.py --baseline a.json b.json --markdown profiles/rotation_ab.md
    python tools/bench_rotation.py --record new.json --baseline a.json b.json --markdown ...   # the table from saved records (no GPU)
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to measure (default: this one)")
ap.add_argument("--legs", default="both", choices=["both", "plain"])
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--angle", type=float, default=0.6)
ap.add_argument("--json", default=None, help="write the record here too")
ap.add_argument("--baseline", nargs="*", default=[], help="records of --legs plain runs of the parent commit, same session")
ap.add_argument("--markdown", default=None, help="write the A/B table here")
ap.add_argument("--note", default=None, help="a closing line for the table's file, e.g. the order the runs were made in")
ap.add_argument("--record", default=None, help="a saved record of this checkout's legs: measure nothing, only write the table")
args = ap.parse_args()
WORKLOAD = "taekwondo-1080p-64+64"


def write_markdown(rec, base, path):
    mean = lambda xs: sum(xs) / len(xs)
    row = lambda name, d: (f"| {name} | {', '.join(f'{x:.1f}' for x in d['frame_ms'])} | {d['frame_ms_mean']:.1f} | {mean(d['sample_coarse_ms']):.3f} | "
                           f"{mean(d['resample_ms']):.3f} | {mean(d['mlp_stage_ms']):.1f} |")
    lines = ["# Per-layer rotation: A/B on the headline shape", "",
             f"`tools/bench_rotation.py`: {WORKLOAD}, split bf16, one MI355X, whole view per frame; {rec['warmup']} warm-up frame(s) per leg, then "
             f"{rec['frames']} frames per leg (frame i from pose i: the columns of a row are different poses, the rows share them), unrotated and "
             f"rotated (performer 1 by {rec.get('angle', 0.6)} rad about z through its box centre) alternating in one process, every frame under the "
             "launch profiler.  Kernel columns: the frame's summed launches, mean over the frames, in ms.", "",
             "| leg | frame ms (pose 0, 1, 2) | mean | sample_coarse | resample | mlp_stage |", "|---|---|---|---|---|---|"]
    for k, b in enumerate(base):
        lines.append(row(f"parent commit, unrotated, run {k + 1}", b["plain"]))
    lines.append(row("this commit, unrotated", rec["plain"]))
    if "rotated" in rec:
        lines.append(row("this commit, performer 1 rotated", rec["rotated"]))
    lines += ["", "Ray-bias kernel at op level, one launch piece of 2^19 rays with every ray listed (the pipeline lists a performer's hit rays only; "
              "its launches have no profiler record of their own, the stage's covers them), ms: "
              + "; ".join([f"parent run {k + 1} {b['ray_bias_plain_ms']:.4f}" for k, b in enumerate(base)]
                          + [f"this commit plain {rec['ray_bias_plain_ms']:.4f}"]
                          + ([f"rotated {rec['ray_bias_rotated_ms']:.4f}"] if "rotated" in rec else [])) + "."]
    if base:
        poses = range(len(rec["plain"]["frame_ms"]))
        per_pose = [[b["plain"]["frame_ms"][i] for b in base] for i in poses]
        spread = [max(x) - min(x) for x in per_pose]
        delta = [rec["plain"]["frame_ms"][i] - mean(per_pose[i]) for i in poses]
        pmean = mean([b["plain"]["frame_ms_mean"] for b in base])
        lines += ["", f"Spread of the parent's unrotated frames in this session (the same pose in its {len(base)} runs): "
                  f"{', '.join(f'{x:.1f}' for x in spread)} ms, at most {100 * max(spread) / pmean:.2f} % of a frame.  This commit's unrotated frames "
                  f"against the parent's mean of the same pose: {', '.join(f'{x:+.1f}' for x in delta)} ms (mean {rec['plain']['frame_ms_mean'] - pmean:+.1f} ms, "
                  f"{100 * (rec['plain']['frame_ms_mean'] - pmean) / pmean:+.2f} %), of which "
                  f"{mean(rec['plain']['mlp_stage_ms']) - mean([mean(b['plain']['mlp_stage_ms']) for b in base]):+.1f} ms are the network stages, whose "
                  "kernels this commit does not touch (the runs follow one another on a socket at its power limit)."]
    if "rotated" in rec:
        d = rec["rotated"]["frame_ms_mean"] - rec["plain"]["frame_ms_mean"]
        lines += ["", f"Rotated against unrotated, this commit: {d:+.1f} ms per frame ({100 * d / rec['plain']['frame_ms_mean']:+.2f} %), of which "
                  f"{mean(rec['rotated']['mlp_stage_ms']) - mean(rec['plain']['mlp_stage_ms']):+.1f} ms are the network stages: the turned performer is hit by "
                  "other rays (the stage kernels and their work per listed row are the same), which is scene content, not the cost of the feature.  The kernels the feature touches: sampler "
                  f"{mean(rec['rotated']['sample_coarse_ms']) - mean(rec['plain']['sample_coarse_ms']):+.3f} ms, resampler "
                  f"{mean(rec['rotated']['resample_ms']) - mean(rec['plain']['resample_ms']):+.3f} ms per frame (a rotated call runs the resampler flavour that "
                  "carries the box edits instead of the specialised production one), ray bias as above."]
    if args.note:
        lines += ["", args.note]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if args.record:
    write_markdown(json.load(open(args.record)), [json.load(open(p)) for p in args.baseline], args.markdown)
    sys.exit(0)

sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

import bench  # noqa: E402
from stnerf_amd import ops, synthetic as syn  # noqa: E402
from stnerf_amd.parallel import render_view  # noqa: E402

model, (H, W, L, n1, n2, st, dt) = bench.build_scene(WORKLOAD, "cuda")
model.set_precision("bf16x3")
frame_ids = [1.0] + [2.5] * L


def frame(i, rotation):
    """One view under the profiler -> (ms, {kernel: summed ms})."""
    if rotation is not None:
        model.rotation = rotation
    K, T = syn.camera(H, W, orbit_deg=10.0 + 1.5 * i)
    model.seed = i
    torch.cuda.synchronize()
    ops.profile_begin()
    t0 = time.perf_counter()
    with torch.no_grad():
        render_view(model, K, T, H, W, frame_ids)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    per = {}
    for r in ops.profile_end():
        per[r["kernel"]] = per.get(r["kernel"], 0.0) + r["ms"]
    if rotation is not None:
        model.rotation = None
    return ms, per


rotated = [None, args.angle] + [None] * (L - 1)
legs = {"plain": [], "rotated": []}
for i in range(args.warmup):
    frame(-1 - i, None)
    if args.legs == "both":
        frame(-1 - i, rotated)
for i in range(args.frames):             # the same pose for the two legs of a pair
    legs["plain"].append(frame(i, None))
    if args.legs == "both":
        legs["rotated"].append(frame(i, rotated))


def ray_bias_ms(rotation):
    """The ray-bias kernel on one launch piece of 2^19 rays, every ray listed (the pipeline lists a performer's hit rays only)."""
    n = 1 << 19
    g = torch.Generator(device="cuda").manual_seed(1)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, device="cuda", generator=g), dim=-1)
    times = torch.full((n,), 2.5, device="cuda")
    net = model.spacenets[0]._packed("fp32")
    kw = {} if rotation is None else dict(rotations=rotation)
    for _ in range(2):
        ops.rgb_ray_bias(net, dirs, times, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        ops.rgb_ray_bias(net, dirs, times, **kw)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 5          # (includes the output's memset of the op wrapper, the same in both)


def digest(rows):
    ms = [r[0] for r in rows]
    kern = lambda k: [round(r[1].get(k, 0.0), 3) for r in rows]
    return dict(frame_ms=[round(x, 2) for x in ms], frame_ms_mean=round(sum(ms) / len(ms), 2), sample_coarse_ms=kern("sample_coarse"),
                resample_ms=kern("resample"), mlp_stage_ms=kern("mlp_stage"), composite_ms=kern("composite"))


rec = dict(workload=WORKLOAD, precision="bf16x3", frames=args.frames, warmup=args.warmup, tree=os.path.basename(os.path.abspath(args.tree)),
           plain=digest(legs["plain"]), ray_bias_plain_ms=round(ray_bias_ms(None), 4))
if args.legs == "both":
    import math
    m = torch.tensor([[math.cos(args.angle), math.sin(args.angle), 0.0], [-math.sin(args.angle), math.cos(args.angle), 0.0], [0.0, 0.0, 1.0]])
    rec.update(angle=args.angle, rotated=digest(legs["rotated"]), ray_bias_rotated_ms=round(ray_bias_ms((m, None)), 4))
print(json.dumps(rec))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rec, f)

if args.markdown:
    write_markdown(rec, [json.load(open(p)) for p in args.baseline], args.markdown)
