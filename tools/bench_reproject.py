"""Reprojection of the background across nearby views (stnerf_amd.reproject) on a bench.py workload: what
a short camera path costs plainly and with key plates every 4 and 8 frames, and what the frames look like.

    python tools/bench_reproject.py [--workload taekwondo-1080p-64+64] [--poses 16] [--degrees 4] [--md profiles/reproject_ab.md]
    python tools/bench_reproject.py --legs "plain,key_every 4,exclusive" --no-sweep --md profiles/reproject_exclusive_ab.md

An orbit path of ``--poses`` poses over ``--degrees`` degrees in total from bench.py's first camera (orbit 10 degrees, frame ids
1 / 2.5, thresholds 0), rendered in one process by three ``LayeredNeuralRenderer``s over the same model -- plain, key_every 4,
key_every 8 -- and a fourth, ``exclusive`` (key_every 4 with ``ReprojectSpec(exclusive=True)``: one source of background per ray, the
networks only where the plate has no row) -- INTERLEAVED pose by pose, each frame between device events; ``--legs`` picks a subset.  Per leg: seconds per frame (the key plates a frame
had to render are inside its time), the hole fraction per frame, and the PSNR of every reprojected frame against the plain
render of the same pose.  Then a small sweep of ``rel`` and ``a_min`` on the first in-between poses (PSNR against hole
fraction), and the three kernels alone against their traffic floor (12 B per source pixel, 4 C + 12 B per destination pixel).
Reported, not asserted: the synthetic scene is a random-weight fog, not a surface -- most of its background rays composite to an
alpha far below any useful a_min, and one depth per pixel describes a fog badly.
Prints a markdown report (also to --md) and ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--degrees", type=float, default=4.0, help="the orbit the whole path covers")
    ap.add_argument("--rel", type=float, default=None, help="the legs' guard (default: the package's)")
    ap.add_argument("--a-min", type=float, default=None, help="the legs' alpha floor (default: the package's)")
    ap.add_argument("--sweep-rel", default="0.02,0.05,0.2")
    ap.add_argument("--sweep-a-min", default="0.1,0.5,0.9")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--legs", default="plain,key_every 4,key_every 8,exclusive", help="the legs to run, comma-separated; plain is always run")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, reproject as rp, synthetic as syn
    from stnerf_amd.render import LayeredNeuralRenderer
    if not torch.cuda.is_available():
        sys.exit("bench_reproject.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.fresh_draws_per_call, model.seed = False, 0
    rel = rp.DEFAULT_REL if args.rel is None else args.rel
    a_min = rp.DEFAULT_A_MIN if args.a_min is None else args.a_min
    step = args.degrees / max(args.poses - 1, 1)
    cams = [syn.camera(H, W, orbit_deg=args.orbit_deg + step * i) for i in range(args.poses)]
    cfg = types.SimpleNamespace(DATASETS=types.SimpleNamespace(LAYER_NUM=L, FRAME_NUM=3, FRAME_OFFSET=0),
                                INPUT=types.SimpleNamespace(SIZE_TEST=[W, H]), OUTPUT_DIR="")
    pairs = [(0, 1.0)] + [(i, 2.5) for i in range(1, L + 1)]

    def renderer(**kw):
        r = LayeredNeuralRenderer(cfg, model=model, gt_poses=torch.stack([torch.as_tensor(T) for _, T in cams]), gt_Ks=[K for K, _ in cams], **kw)
        r.set_path_gt_poses()
        r.layer_frame_pairs = [list(pairs) for _ in cams]               # bench.py's frame ids on every pose: the camera alone moves
        return r

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / 1e3, out

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, poses=args.poses,
                             degrees=args.degrees, rel=rel, a_min=a_min, command=" ".join(["python", "tools/bench_reproject.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}; {args.poses} poses over {args.degrees} degrees "
        f"({step:.3f} per pose) from orbit {args.orbit_deg}; rel {rel}, a_min {a_min}.")
    say()
    specs = {"key_every 4": dict(key_every=4), "key_every 8": dict(key_every=8), "exclusive": dict(key_every=4, exclusive=True)}
    wanted = [x.strip() for x in args.legs.split(",") if x.strip() and x.strip() != "plain"]
    if any(x not in specs for x in wanted):
        sys.exit(f"--legs: choose from plain, {', '.join(specs)}")
    legs = [("plain", renderer())] + [(x, renderer(reproject=dict(rel=rel, a_min=a_min, **specs[x]))) for x in wanted]
    timed(lambda: legs[0][1]._render_frame(0, 0, 0, False))             # warm-up: packs, workspace, clocks
    seconds = {name: [] for name, _ in legs}
    quality = {name: [] for name, _ in legs[1:]}
    plain_frames = {}
    for idx in range(args.poses):                                       # interleaved: the three legs of a pose back to back
        ref = None
        for name, r in legs:
            s, out = timed(lambda: r._render_frame(idx, 0, 0, False))
            seconds[name].append(s)
            if name == "plain":
                ref = out[0]
                if idx < 4:
                    plain_frames[idx] = ref.clone()
            else:
                quality[name].append(psnr(out[0], ref))
    say("| leg | s / frame (mean) | median | min .. max | x of plain | holes / frame (mean, min .. max) | key plates rendered | PSNR vs plain (mean, min .. max) |")
    say("|---|---|---|---|---|---|---|---|")
    base = statistics.mean(seconds["plain"])
    result["legs"] = {}
    for name, r in legs:
        s = seconds[name]
        row = dict(seconds=s, mean_s=statistics.mean(s), median_s=statistics.median(s))
        if name == "plain":
            say(f"| plain | {row['mean_s']:.3f} | {row['median_s']:.3f} | {min(s):.3f} .. {max(s):.3f} | 1.000 | | | |")
        else:
            holes = [x["holes"] / (H * W) for x in r.reproject_stats]
            keys = sum(x["keys_rendered"] for x in r.reproject_stats)
            q = quality[name]
            row.update(hole_fraction=holes, keys_rendered=keys, psnr=q)
            say(f"| {name} | {row['mean_s']:.3f} | {row['median_s']:.3f} | {min(s):.3f} .. {max(s):.3f} | {row['mean_s'] / base:.3f} | "
                f"{statistics.mean(holes):.4f}, {min(holes):.4f} .. {max(holes):.4f} | {keys} | {statistics.mean(q):.2f}, {min(q):.2f} .. {max(q):.2f} dB |")
        result["legs"][name] = row
    say()
    if "exclusive" in seconds:
        # the in-between frames alone (a key frame carries its plates' renders): what the mode was built for
        r = dict(legs)["exclusive"]
        between = [i for i, x in enumerate(r.reproject_stats) if x["keys_rendered"] == 0]
        mean_of = lambda name: statistics.mean(seconds[name][i] for i in between)
        line = (f"`exclusive` is key_every 4 with one source of background per ray.  Whole path: {statistics.mean(seconds['exclusive']) / base:.3f} x "
                f"plain.  In-between frames only ({len(between)} of {args.poses}, no key plate rendered): exclusive {mean_of('exclusive'):.3f} s, "
                f"plain {mean_of('plain'):.3f} s ({mean_of('exclusive') / mean_of('plain'):.3f} x)")
        if "key_every 4" in seconds:
            line += (f", key_every 4 {mean_of('key_every 4'):.3f} s ({mean_of('exclusive') / mean_of('key_every 4'):.3f} x of it); whole path "
                     f"{statistics.mean(seconds['exclusive']) / statistics.mean(seconds['key_every 4']):.3f} x of key_every 4")
        flagged = statistics.mean(r.reproject_stats[i]["holes"] / (H * W) for i in between)
        say(line + f".  Flagged rays (holes and plate rows below a_min) on those frames: {flagged:.4f} of the view.")
        say()
    for name, r in legs[1:]:
        say(f"{name}, per frame (seconds / hole fraction / PSNR dB): "
            + "; ".join(f"{s:.2f} / {x['holes'] / (H * W):.3f} / {q:.1f}" for s, x, q in zip(seconds[name], r.reproject_stats, quality[name])))
        say()
    say("The yardstick the README quotes for this scene: the device-RNG render against itself across draws, 31.6 dB.  The scene is a "
        "random-weight fog, not a surface: the PSNR above is reported, not asserted.")
    say()
    if not args.no_sweep:
        result["sweep"] = sweep(args, say, model, parallel, rp, cams, H, W, [p[1] for p in pairs], plain_frames, timed)
    result.update(kernels_of(say, ops, rp, model, cams, H, W, [p[1] for p in pairs], rel, a_min, base, device))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


def sweep(args, say, model, parallel, rp, cams, H, W, ids, plain_frames, timed):
    """rel x a_min on poses 1..3 warped from the key at pose 0: PSNR against hole fraction."""
    say("Sweep (one key at pose 0; poses 1, 2, 3 warped from it; mean over the three):")
    say()
    say("| a_min | rel | plate rows present | holes / frame | PSNR vs plain | s / frame |")
    say("|---|---|---|---|---|---|")
    rows = []
    for a_min in [float(x) for x in args.sweep_a_min.split(",")]:
        plate = None
        for rel in [float(x) for x in args.sweep_rel.split(",")]:
            spec = rp.ReprojectSpec(4, rel, a_min)
            if plate is None:
                plate = rp.BackgroundPlate.render(model, cams[0][0], cams[0][1], H, W, ids, spec, index=0)
            present = int((plate.t == plate.t).sum()) / (H * W)
            holes, q, secs = [], [], []
            for i in (1, 2, 3):
                if i not in plain_frames:
                    continue
                s, (_, _, occluded, stats) = timed(lambda: parallel.render_view_reprojected(model, cams[i][0], cams[i][1], H, W, ids, [plate], spec))
                holes.append(stats["holes"] / (H * W))
                q.append(psnr(occluded["mixed"][0].reshape(H, W, 3), plain_frames[i]))
                secs.append(s)
            row = dict(a_min=a_min, rel=rel, present=present, hole_fraction=statistics.mean(holes), psnr=statistics.mean(q), seconds=statistics.mean(secs))
            rows.append(row)
            say(f"| {a_min} | {rel} | {present:.4f} | {row['hole_fraction']:.4f} | {row['psnr']:.2f} dB | {row['seconds']:.3f} |")
    say()
    return rows


def kernels_of(say, ops, rp, model, cams, H, W, ids, rel, a_min, frame_s, device):
    """Splat + resolve + hole list alone (two sources into one view), between device events, against the traffic floor."""
    spec = rp.ReprojectSpec(4, rel, a_min)
    plates = [rp.BackgroundPlate.render(model, cams[i][0], cams[i][1], H, W, ids, spec, index=i) for i in (0, min(4, len(cams) - 1))]
    K, T = cams[min(2, len(cams) - 1)]
    sources = [p.source() for p in plates]
    ops.reproject(sources, K, T, H, W, rel)
    ms = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ops.reproject(sources, K, T, H, W, rel)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    floor = (12 * len(sources) + 4 * 5 + 12) * H * W
    med = statistics.median(ms)
    say(f"The kernels alone (`ops.reproject`: {len(sources)} splats, resolve, three launches of the hole list, the fill of the keys and one "
        f"D2H; {H * W} pixels, C = 5): median {med:.3f} ms of 10 between device events ({min(ms):.3f} .. {max(ms):.3f}); traffic floor "
        f"12 B per source pixel + (4 C + 12) B per destination pixel = {floor / 1e6:.1f} MB -> {floor / 1e9 / (med / 1e3):.0f} GB/s; "
        f"{100 * med / 1e3 / frame_s:.3f} % of a plain frame ({frame_s:.3f} s).")
    say()
    return dict(kernels_ms=ms, kernels_floor_MB=floor / 1e6)


if __name__ == "__main__":
    main()
