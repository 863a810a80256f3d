"""A/B of the background's occupancy grid (stnerf_amd.OccupancyGrids.set_background_manual) on a bench.py
workload's frame.

    python tools/bench_background_grid.py [--workload taekwondo-1080p-64+64] [--reps 3] [--md out.md]

The method is tools/bench_sample_cull.py's: one camera, one frame, rendered in one process under the variants below, interleaved,
`--reps` repetitions each after a warm-up:
  (a)    no grid;
  (o)    an all-ones background grid, 8 cells a side: every sample is listed, so what it costs over (a) is the two rows launches and
         the row-list flavour of the stage kernels;
  (r64)  a manual "room" grid over `bkgd_bbox`, 64 cells a side: occupied are the cells within two cells of the box's walls (both
         ends of x and of y) and of its floor (the low end of z);
  (r256) the same room at 256 cells a side (a 2 MB bit table).
Reported: frame times, background samples tested / skipped over both stages, the frame's network rows against (a) (the background's
on every ray + the performers' on their hit rays), the PSNR of every frame against (a) on the same draws, and the two rows launches'
time and bytes from the library's launch profiler.  Prints a markdown report (also to --md) and ONE JSON line.
The synthetic background is a dense random field, not a room: a grid BUILT from the networks lists nearly everything, and under the
manual room grid the picture differs a lot from (a).  The run measures what the cull saves per skipped row, not a picture."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * math.log10(mse)


def room(res, shell=2):
    """bool [Rz][Ry][Rx]: the cells within ``shell`` cells of the walls (both ends of x and y) and of the floor (low z)."""
    z, y, x = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing="ij")
    return torch.from_numpy((x < shell) | (x >= res - shell) | (y < shell) | (y >= res - shell) | (z < shell))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.occupancy import OccupancyGrids, box_bounds
    if not torch.cuda.is_available():
        sys.exit("bench_background_grid.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [1.0 + (0.5 * i + 0.25) % 2 for i in range(L)]           # fractional performer frame ids
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.seed, model.fresh_draws_per_call = 0, False
    lo, hi = box_bounds(model.bkgd_bbox)

    def manual(occupied):
        g = OccupancyGrids(auto=False)
        g.set_background_manual(occupied, lo, hi)
        return g

    def frame(grids):
        model.set_occupancy(grids)
        if grids is not None:
            grids.reset_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        model.set_occupancy(None)
        hit_pairs = sum(int(m.sum()) for m in out[4][1:])
        return dt_s, out[0][0], (grids.stats() if grids is not None else None), hit_pairs

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frame_ids=ids,
                             command=" ".join(["python", "tools/bench_background_grid.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}; background box {lo.tolist()} .. {hi.tolist()}; "
        "room grids: the cells within two cells of the walls (x, y) and the floor (low z).")
    say()
    built = {"a": None, "o": manual(torch.ones(8, 8, 8, dtype=torch.bool)), "r64": manual(room(64)), "r256": manual(room(256))}
    frame(None)                                                         # warm-up: packs, workspace, clocks
    frame(built["r256"])                                                # ... and the larger workspace of the row list
    times, stats, images, pairs = {k: [] for k in built}, {}, {}, 0
    for _ in range(args.reps):
        for name in built:
            t, img, st_, pairs = frame(built[name])
            times[name].append(t)
            stats[name], images[name] = st_, img
    per_pair = 2 * n1 + n2
    full_rows = (H * W + pairs) * per_pair
    say("| variant | frame s (median) | min .. max | vs (a) | background samples tested / skipped (both stages) | listed of tested | rows evaluated vs (a) | PSNR vs (a) |")
    say("|---|---|---|---|---|---|---|---|")
    rows = {}
    for name in built:
        tested, skipped = (stats[name] or {}).get("background", (0, 0))
        rows[name] = dict(median_s=statistics.median(times[name]), min_s=min(times[name]), max_s=max(times[name]), tested=tested, skipped=skipped,
                          network_rows=full_rows - skipped, psnr_vs_a=None if name == "a" else psnr(images[name], images["a"]))
    for name, r in rows.items():
        say(f"| ({name}) | {r['median_s']:.3f} | {r['min_s']:.3f} .. {r['max_s']:.3f} | x{rows['a']['median_s'] / r['median_s']:.3f} | "
            + (f"{r['tested']} / {r['skipped']}" if r["tested"] else "-") + " | "
            + (f"{100 * (r['tested'] - r['skipped']) / r['tested']:.1f} %" if r["tested"] else "-") + " | "
            + f"x{r['network_rows'] / full_rows:.4f} | " + ("-" if name == "a" else f"{r['psnr_vs_a']:.2f} dB") + " |")
    say()
    say("Time against rows: " + "; ".join(f"({k}) / (a) = {rows[k]['median_s'] / rows['a']['median_s']:.4f} of the time for "
                                          f"{rows[k]['network_rows'] / full_rows:.4f} of the rows" for k in ("o", "r64", "r256")) + ".")
    for name in ("r64", "r256"):                                        # the two rows launches of one frame, timed by the library's profiler
        model.set_occupancy(built[name])
        built[name].reset_stats()
        ops.profile_begin()
        parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        recs = ops.profile_end()
        model.set_occupancy(None)
        tested, skipped = built[name].stats()["background"]
        rk = [r for r in recs if r["kernel"] == "background_rows"]
        rows_ms, all_ms = sum(r["ms"] for r in rk), sum(r["ms"] for r in recs)
        by_ns = {ns: sum(r["ms"] for r in rk if r["ns"] == ns) for ns in sorted({r["ns"] for r in rk})}
        rows_bytes = 12 * tested + 16 * skipped + 4 * (tested - skipped)
        say(f"Rows launches of one ({name}) frame: {len(rk)} launches, {rows_ms:.3f} ms of {all_ms:.1f} ms launch time ({100 * rows_ms / all_ms:.3f} %), "
            + ", ".join(f"{ms:.3f} ms at ns = {ns}" for ns, ms in by_ns.items())
            + f"; {rows_bytes / 1e9:.3f} GB (12 B read per tested sample, 16 B written per skipped one, 4 B per listed one) = "
            f"{rows_bytes / 1e9 / max(rows_ms / 1e3, 1e-9):.0f} GB/s.")
        rows[name].update(rows_ms=rows_ms, launch_ms=all_ms, rows_ms_by_ns=by_ns, rows_GB=rows_bytes / 1e9)
    say()
    result.update(variants=rows, full_rows=full_rows, hit_pairs=pairs)
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
