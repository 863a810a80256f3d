#!/usr/bin/env python3
"""What the in-scene layer passes cost (GPU box): the bench's headline shape (taekwondo-1080p-64+64, split bf16, one GPU), frames
without and with the pass (``render_view(..., scene=True)``) ALTERNATING in one process, three each after the warm-up, every frame
under the library's launch profiler (ops.profile_begin / profile_end).  Reports per leg the frame times and the frame's summed
compositor launches (with the pass: the merged-weight stores and layer_scene_kernel are inside that record).

The bar that matters is the render WITHOUT the pass: the compositor launches of such a render must not slow down.  That is
measured at op level with tools/bench_composite.py, the parent commit and this one alternating; this tool reads the logs of those
runs and writes both comparisons into one file.

    python tools/bench_scene_passes.py                                  # both legs of this checkout -> JSON on stdout
    python tools/bench_scene_passes.py --tree DIR --legs plain --json a.json    # the leg without the pass of ANOTHER checkout (built
                                                                                # in place), e.g. the parent commit
    python tools/bench_scene_passes.py --record new.json --baseline a.json --composite-parent p1.log p2.log p3.log \\
        --composite-this t1.log t2.log t3.log --markdown profiles/scene_passes_ab.md      # the tables from saved records (no GPU)
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to measure (default: this one)")
ap.add_argument("--legs", default="both", choices=["both", "plain"])
ap.add_argument("--frames", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--json", default=None, help="write the record here too")
ap.add_argument("--baseline", nargs="*", default=[], help="records of --legs plain runs of the parent commit, same session")
ap.add_argument("--composite-parent", nargs="*", default=[], help="outputs of tools/bench_composite.py on the parent commit, same session")
ap.add_argument("--composite-this", nargs="*", default=[], help="outputs of tools/bench_composite.py on this commit, alternating with the parent's")
ap.add_argument("--markdown", default=None, help="write the A/B tables here")
ap.add_argument("--note", default=None, help="a closing line for the table's file, e.g. the order the runs were made in")
ap.add_argument("--record", default=None, help="a saved record of this checkout's legs: measure nothing, only write the tables")
args = ap.parse_args()
WORKLOAD = "taekwondo-1080p-64+64"


def composite_log(path):
    """{case: ms} of one tools/bench_composite.py run."""
    out = {}
    for line in open(path):
        m = re.match(r"\s*\w+\s+(.+?)\s+n=\s*\d+ live layers/ray\s+[\d.]+:\s+([\d.]+) ms", line)
        if m:
            out[m.group(1).strip()] = float(m.group(2))
    return out


def write_markdown(rec, base, path):
    mean = lambda xs: sum(xs) / len(xs)
    row = lambda name, d: (f"| {name} | {', '.join(f'{x:.1f}' for x in d['frame_ms'])} | {d['frame_ms_mean']:.1f} | {mean(d['composite_ms']):.3f} | "
                           f"{mean(d['mlp_stage_ms']):.1f} |")
    lines = ["# In-scene layer passes: cost with the pass on, and the compositor with it off", "",
             "## A frame with and without the pass", "",
             f"`tools/bench_scene_passes.py`: {WORKLOAD}, split bf16, one MI355X, whole view per frame; {rec['warmup']} warm-up frame(s) per leg, "
             f"then {rec['frames']} frames per leg (frame i from pose i: the rows share the poses), without and with the pass alternating in one "
             "process, every frame under the launch profiler.  Kernel columns: the frame's summed launches, mean over the frames, in ms; with the "
             "pass the compositor's record includes the merged-weight stores and `layer_scene_kernel`.", "",
             "| leg | frame ms (pose 0, 1, 2) | mean | composite | mlp_stage |", "|---|---|---|---|---|"]
    for k, b in enumerate(base):
        lines.append(row(f"parent commit, run {k + 1}", b["plain"]))
    lines.append(row("this commit, pass off", rec["plain"]))
    if "scene" in rec:
        lines.append(row("this commit, pass on", rec["scene"]))
        dc = mean(rec["scene"]["composite_ms"]) - mean(rec["plain"]["composite_ms"])
        df = rec["scene"]["frame_ms_mean"] - rec["plain"]["frame_ms_mean"]
        lines += ["", f"The pass costs {dc:+.3f} ms of compositor time per frame ({100 * dc / rec['plain']['frame_ms_mean']:+.3f} % of a frame); the frames "
                  f"differ by {df:+.1f} ms ({100 * df / rec['plain']['frame_ms_mean']:+.2f} %), the rest being the network stages' run-to-run noise."]
    cp, ct = [composite_log(p) for p in args.composite_parent], [composite_log(p) for p in args.composite_this]
    if cp and ct:
        lines += ["", "## The compositor alone, pass off: parent against this commit", "",
                  f"`tools/bench_composite.py` (`ops.composite`, production kernels, ms per call), {len(cp)} runs of the parent commit and {len(ct)} of this "
                  "one alternating on one MI355X.  The instantiations a call without the pass launches are the parent's instruction for instruction "
                  "(`tests/test_scene_passes_cpu.py` holds their registers).", "",
                  "| case | parent runs | parent median | parent spread | this commit runs | this median | median - median |", "|---|---|---|---|---|---|---|"]
        inside = []
        for case in cp[0]:
            a, b = [r[case] for r in cp if case in r], [r[case] for r in ct if case in r]
            if not b:
                continue
            ma, mb = statistics.median(a), statistics.median(b)
            inside.append(min(a) <= mb <= max(a))
            lines.append(f"| {case} | {', '.join(f'{x:.3f}' for x in a)} | {ma:.3f} | {max(a) - min(a):.3f} | {', '.join(f'{x:.3f}' for x in b)} | {mb:.3f} | "
                         f"{mb - ma:+.3f} |")
        lines += ["", f"This commit's median lies inside the parent's own min .. max in {sum(inside)} of {len(inside)} cases."]
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


def frame(i, scene):
    """One view under the profiler -> (ms, {kernel: summed ms})."""
    K, T = syn.camera(H, W, orbit_deg=10.0 + 1.5 * i)
    model.seed = i
    torch.cuda.synchronize()
    ops.profile_begin()
    t0 = time.perf_counter()
    with torch.no_grad():
        render_view(model, K, T, H, W, frame_ids, **(dict(scene=True) if scene else {}))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    per = {}
    for r in ops.profile_end():
        per[r["kernel"]] = per.get(r["kernel"], 0.0) + r["ms"]
    return ms, per


legs = {"plain": [], "scene": []}
for i in range(args.warmup):
    frame(-1 - i, False)
    if args.legs == "both":
        frame(-1 - i, True)
for i in range(args.frames):             # the same pose for the two legs of a pair
    legs["plain"].append(frame(i, False))
    if args.legs == "both":
        legs["scene"].append(frame(i, True))


def digest(rows):
    ms = [r[0] for r in rows]
    kern = lambda k: [round(r[1].get(k, 0.0), 3) for r in rows]
    return dict(frame_ms=[round(x, 2) for x in ms], frame_ms_mean=round(sum(ms) / len(ms), 2), composite_ms=kern("composite"),
                mlp_stage_ms=kern("mlp_stage"))


rec = dict(workload=WORKLOAD, precision="bf16x3", frames=args.frames, warmup=args.warmup, tree=os.path.basename(os.path.abspath(args.tree)),
           plain=digest(legs["plain"]))
if args.legs == "both":
    rec.update(scene=digest(legs["scene"]))
print(json.dumps(rec))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rec, f)

if args.markdown:
    write_markdown(rec, [json.load(open(p)) for p in args.baseline], args.markdown)
