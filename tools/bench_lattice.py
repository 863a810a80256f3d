"""Adaptive lattice frames (stnerf_amd.lattice) on a bench.py workload's frame: what the sparse lattice saves
and what it costs in the picture.

    python tools/bench_lattice.py [--workload taekwondo-1080p-64+64] [--tols auto | t1,t2,t3] [--levels 2,3] [--reps 2] [--md out.md]

One camera, one frame (bench.py's first step: orbit 10 degrees, frame ids 1 / 2.5, thresholds 0), rendered in one process, the
legs interleaved round after round:
  the plain ``render_view``, and lattice frames at every ``--levels`` K and three values of ``tol_rgb``
(``--tols auto``: the 25 %, 50 % and 75 % quantiles over the top-level cells (stride 2^max K) of the plain frame of the corner
spread of their colour columns, the largest one).  ``force`` is the default, "performers".  For each leg: seconds (the median
over the rounds), rays rendered per level, the filled fraction, and PSNR and the largest absolute error of the mixed colour
against the plain frame -- which a lattice frame cannot equal even where it renders: a ray of a sparse list draws its jitter by
its place in the list.  Then the lattice launches alone (begin, select + scatter, classify per stride), timed with device events
on a state as large as the frame's.  Reported, not asserted: the scene is a dense synthetic random field, and what a real
background allows nobody has measured.
Prints a markdown report (also to --md) and ONE JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def cell_spread(packed, H, W, levels, l):
    """(cells,) on the device: per top-level cell of a full frame (n, 6 + 5 l), the largest corner spread of its colour columns."""
    from stnerf_amd.lattice import covered
    S = 1 << levels
    Wc, Hc = covered(H, W, levels)
    cols = [c for c in range(5 + 5 * l) if c % 5 < 3]
    img = packed.reshape(H, W, -1)[:Hc + 1:S, :Wc + 1:S][:, :, cols]
    four = torch.stack([img[:-1, :-1], img[:-1, 1:], img[1:, :-1], img[1:, 1:]], 0)
    return (four.max(0)[0] - four.min(0)[0]).max(-1)[0].reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--levels", default="2,3", help="the K of the lattice legs")
    ap.add_argument("--tols", default="auto", help="three values of tol_rgb t1,t2,t3, or auto: quantiles of the top-level cells' corner spread")
    ap.add_argument("--reps", type=int, default=2, help="rounds over all legs after the warm-up round")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.lattice import LatticeSpec
    if not torch.cuda.is_available():
        sys.exit("bench_lattice.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [2.5] * L
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.fresh_draws_per_call = False
    l = parallel.total_layers(model)
    levels = [int(k) for k in args.levels.split(",")]

    def plain_frame():
        model.seed = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def lattice_frame(spec):
        model.seed = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, stats = parallel.render_view_lattice(model, K, T, H, W, ids, spec, device=device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, stats

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=l,
                             command=" ".join(["python", "tools/bench_lattice.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}; a synthetic scene (bench.py's: a dense random "
        "field), force = \"performers\".")
    say()
    _, plain = plain_frame()                                            # warm-up: packs, workspace, clocks
    packed = torch.cat(list(plain[0]) + [x for t in plain[2] for x in t], 1)
    spread = cell_spread(packed, H, W, max(levels), l)
    quartiles = [float(torch.quantile(spread, q)) for q in (0.25, 0.5, 0.75)]
    tols = quartiles if args.tols == "auto" else [float(x) for x in args.tols.split(",")]
    legs = [(f"K = {k}, tol_rgb {t:.3e}", LatticeSpec(k, t)) for k in levels for t in tols]
    lattice_frame(legs[0][1])                                           # warm-up of the lattice launches
    seconds = {name: [] for name, _ in [("plain", None)] + legs}
    kept = {}
    for _ in range(max(1, args.reps)):
        t, plain = plain_frame()
        seconds["plain"].append(t)
        for name, spec in legs:
            t, out, stats = lattice_frame(spec)
            seconds[name].append(t)
            kept[name] = (out, stats)
    t_plain = statistics.median(seconds["plain"])
    say(f"`render_view` of the frame: median {t_plain:.3f} s of {len(seconds['plain'])} ({min(seconds['plain']):.3f} .. {max(seconds['plain']):.3f}).  "
        f"Corner spread of the colour columns over the {spread.numel()} cells of stride {1 << max(levels)} of the plain frame: quartiles "
        + " / ".join(f"{q:.3e}" for q in quartiles) + ".")
    say()
    say("| frame | seconds (median) | x of plain | rays rendered per level | rendered | filled | forced | PSNR vs plain | max abs error |")
    say("|---|---|---|---|---|---|---|---|---|")
    rows = []
    for name, spec in legs:
        out, stats = kept[name]
        t = statistics.median(seconds[name])
        row = dict(frame=name, levels=spec.levels, tol_rgb=spec.tol_rgb, seconds=t, seconds_all=seconds[name], ratio=t / t_plain,
                   rays_per_level=stats["rays_per_level"], rendered_fraction=stats["rendered"] / (H * W),
                   filled_fraction=stats["filled"] / (H * W), forced_fraction=stats["forced"] / (H * W), margin=stats["margin"],
                   psnr_vs_plain=psnr(out[0][0], plain[0][0]), max_abs_error=float((out[0][0] - plain[0][0]).abs().max()))
        rows.append(row)
        say(f"| {name} | {t:.3f} | {row['ratio']:.3f} | {row['rays_per_level']} | {100 * row['rendered_fraction']:.2f} % | "
            f"{100 * row['filled_fraction']:.2f} % | {100 * row['forced_fraction']:.2f} % | {row['psnr_vs_plain']:.2f} dB | {row['max_abs_error']:.3e} |")
    say()
    t0, all_pixels, _ = lattice_frame(LatticeSpec(0, 0.0))
    say(f"levels = 0 equals `render_view` of the frame bit for bit: {bool(torch.equal(plain[0][0], all_pixels[0][0]))} ({t0:.3f} s).")
    say()
    result.update(render_view_s=seconds["plain"], quartiles=quartiles, tols=tols, frames=rows)
    result.update(launches_of(say, ops, packed, plain[4], H, W, l, max(levels), tols[1], t_plain, device))
    best = min(rows, key=lambda r: r["seconds"])
    verdict = (f"Verdict: on this synthetic scene the fastest lattice leg ({best['frame']}) takes {best['ratio']:.2f} x the plain frame's time "
               f"with {100 * best['filled_fraction']:.1f} % of the pixels filled at {best['psnr_vs_plain']:.1f} dB -- "
               + ("a gain." if best["ratio"] < 0.95 else "no gain on this scene."))
    say(verdict)
    result["verdict"] = verdict
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


def launches_of(say, ops, packed, masks, H, W, l, levels, tol_rgb, plain_s, device):
    """The lattice launches alone on a state as large as the frame's, its rows taken from the plain frame: begin, then per level
    select + scatter and classify, each between device events; the whole loop ten times."""
    from stnerf_amd.lattice import LatticeSpec
    spec = LatticeSpec(levels, tol_rgb)
    bits = sum(m.to(torch.float32) * float(1 << i) for i, m in enumerate(masks)).reshape(-1, 1)
    rows = torch.cat([packed, bits], 1).contiguous()
    tol = torch.tensor(spec.tolerances(l), dtype=torch.float32, device=device)
    state = ops.lattice_state(H, W, rows.shape[1], device)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    names = ["begin"] + [x for s in spec.strides() for x in (f"select + scatter before stride {s}", f"classify at stride {s}")] + ["last select + scatter"]
    ms = {n: [] for n in names}
    lists = []

    def timed(name, fn):
        a, b = ev(), ev()
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize()
        ms[name].append(a.elapsed_time(b))
        return r

    def listed():
        pix, n = ops.lattice_select(state)
        ops.lattice_scatter(rows[pix.long()], state, pix)      # (the gather of the rows stands in for the render; it is inside the timing)
        return n

    for _ in range(10):
        lists = []
        timed("begin", lambda: ops.lattice_begin(state, levels))
        for s in spec.strides():
            lists.append(timed(f"select + scatter before stride {s}", listed))
            timed(f"classify at stride {s}", lambda: ops.lattice_classify(state, levels, s, tol))
        lists.append(timed("last select + scatter", listed))
    med = {n: statistics.median(v) for n, v in ms.items()}
    total = sum(med.values())
    say(f"The lattice launches alone (K = {levels}, tol_rgb {tol_rgb:.3e}, no force mask, C = {rows.shape[1]}, rows from the plain frame; lists "
        f"{lists}), medians of 10 between device events: " + "; ".join(f"{n} {v:.3f} ms" for n, v in med.items())
        + f".  Together {total:.3f} ms = {100 * total / 1e3 / plain_s:.3f} % of the plain frame's {plain_s:.3f} s.")
    say()
    return dict(launch_ms=ms, launch_lists=lists, launch_total_ms=total)


if __name__ == "__main__":
    main()
