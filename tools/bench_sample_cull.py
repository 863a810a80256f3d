"""A/B of the sample cull (stnerf_amd.OccupancyGrids(samples=True)) on a bench.py workload's frame.

    python tools/bench_sample_cull.py [--workload taekwondo-1080p-64+64] [--reps 3] [--sparse-bias -3.0] [--md out.md]
    python tools/bench_occupancy.py --tree DIR --legs plain --json parent.json     # variant (a) alone, of the parent commit's checkout
    python tools/bench_sample_cull.py --baseline parent.json [parent2.json ...]    # ... its frame time next to this checkout's (a)

The method and the scenes are tools/bench_occupancy.py's: one camera, one frame, rendered in one process under the variants below,
interleaved, `--reps` repetitions each after a warm-up, on the bench scene and on its SPARSE variant
(`synthetic.make_state_dict(sigma_bias=...)`); the grids are the manual ellipsoid inscribed in each performer's box (pi / 6 of its
volume), 64 cells a side:
  (a)  no grids;
  (b)  ray cull (the ellipsoid grids);
  (c)  ray + sample cull (the same grids, samples=True);
  (b1) ray cull with all-ones grids;
  (c1) ray + sample cull with all-ones grids: every sample is listed, so what it costs over (b1) is the rows kernel and the lost
       MotionNet reuse on the gridded layers (about 2.5 %).
Reported: frame times, pairs tested / culled, samples tested / skipped per stage (the coarse stage's from an only_coarse render of the
same rays and draws), the PSNR of every frame against (a) on the same draws next to the PSNR of (a) against itself under another
seed, and the rows kernel's time and bytes from the library's launch profiler.  The parent commit's (a) comes from
`tools/bench_occupancy.py --legs plain` on its checkout, in a process of its own before and after this run (`--baseline`).
Prints a markdown report (also to --md) and ONE JSON line.  The fields are synthetic random fields, not people."""
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


def ellipsoid(res):
    c = (np.arange(res) + 0.5) / res - 0.5
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return torch.from_numpy((x * x + y * y + z * z) <= 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    ap.add_argument("--baseline", nargs="*", default=[], help="records of `bench_occupancy.py --legs plain` runs of the parent commit, same session")
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--sparse-bias", type=float, default=-3.0, help="sigma_bias of the sparse scene's density heads (the bench scene: 0.5)")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.occupancy import OccupancyGrids, box_bounds
    if not torch.cuda.is_available():
        sys.exit("bench_sample_cull.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [1.0 + (0.5 * i + 0.25) % 2 for i in range(L)]           # fractional performer frame ids

    def scene(sigma_bias=None):
        model, _ = bench.build_scene(args.workload, device)
        if sigma_bias is not None:
            model.load_state_dict({k: v.to(device) for k, v in syn.make_state_dict(L, st, dt, seed=0, sigma_bias=sigma_bias).items()})
        model.max_rays_per_launch = args.rays_per_launch
        model.set_precision(args.precision)
        model.seed, model.fresh_draws_per_call = 0, False
        return model

    def frame(model, grids, seed=0):
        model.set_occupancy(grids)
        model.seed = seed
        if grids is not None:
            grids.reset_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        model.set_occupancy(None)
        return dt_s, out[0][0], (grids.stats() if grids is not None else None)

    def manual(model, occupied, samples):
        g = OccupancyGrids(auto=False, samples=samples)
        for i in range(1, L + 1):
            g.set_manual(i, occupied, *box_bounds(model.layer_box_at(i, ids[i])))
        return g

    def coarse_samples(model, grids):
        """(tested, skipped) of the coarse stage alone: an only_coarse render of the same rays under the same seed."""
        rays = ops.generate_rays(K, T, H, W, frame_ids=ids).to(device)
        model.set_occupancy(grids)
        model.seed = 0
        grids.reset_stats()
        with torch.no_grad():
            model.render_rays_raw(rays, True, 0.0, 0.0, ref_chunk=512 * 7)
        torch.cuda.synchronize()
        model.set_occupancy(None)
        s = grids.stats()["samples"]
        return sum(t for t, _ in s.values()), sum(k for _, k in s.values())

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frame_ids=ids,
                             command=" ".join(["python", "tools/bench_sample_cull.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}, performer frame ids {ids[1:]}; "
        f"grids: the ellipsoid inscribed in each box, 64 cells a side.")
    say()
    for tag, bias in (("bench scene", None), ("sparse scene (sigma_bias %.1f)" % args.sparse_bias, args.sparse_bias)):
        model = scene(bias)
        ones = torch.ones(8, 8, 8, dtype=torch.bool)
        built = {"a": None, "b": manual(model, ellipsoid(64), False), "c": manual(model, ellipsoid(64), True),
                 "b1": manual(model, ones, False), "c1": manual(model, ones, True)}
        frame(model, None)                                              # warm-up: packs, workspace, clocks
        frame(model, built["c"])                                        # ... and the larger workspace of the sample cull
        times, stats, images = {k: [] for k in built}, {}, {}
        for _ in range(args.reps):
            for name in built:
                t, img, st_ = frame(model, built[name])
                times[name].append(t)
                stats[name], images[name] = st_, img
        _, other_seed, _ = frame(model, None, seed=1)
        noise = psnr(other_seed, images["a"])
        say(f"### {tag}")
        say()
        say(f"PSNR of (a) against (a) under another seed (the render's own jitter noise): {noise:.2f} dB.")
        say()
        say("| variant | frame s (median) | min .. max | vs (a) | pairs tested / culled | samples tested / skipped (both stages) | rows evaluated vs (a) | PSNR vs (a) |")
        say("|---|---|---|---|---|---|---|---|")
        rows = {}
        full_rows = None
        for name in built:
            med = statistics.median(times[name])
            pairs = (stats[name] or {}).get("pairs", {})
            samples = (stats[name] or {}).get("samples", {})
            tested, culled = sum(t for t, _ in pairs.values()), sum(c for _, c in pairs.values())
            s_tested, s_skipped = sum(t for t, _ in samples.values()), sum(k for _, k in samples.values())
            rows[name] = dict(median_s=med, min_s=min(times[name]), max_s=max(times[name]), pairs_tested=tested, pairs_culled=culled,
                              samples_tested=s_tested, samples_skipped=s_skipped, psnr_vs_a=None if name == "a" else psnr(images[name], images["a"]))
        # network rows of a frame: the background's on every ray + the performers' on kept pairs, minus the skipped samples
        hit_pairs = rows["b1"]["pairs_tested"]
        per_pair = 2 * n1 + n2
        full_rows = (H * W + hit_pairs) * per_pair
        for name, r in rows.items():
            r["network_rows"] = full_rows - r["pairs_culled"] * per_pair - r["samples_skipped"]
            say(f"| ({name}) | {r['median_s']:.3f} | {r['min_s']:.3f} .. {r['max_s']:.3f} | x{rows['a']['median_s'] / r['median_s']:.3f} | "
                + (f"{r['pairs_tested']} / {r['pairs_culled']}" if r["pairs_tested"] else "-") + " | "
                + (f"{r['samples_tested']} / {r['samples_skipped']}" if r["samples_tested"] else "-") + " | "
                + f"x{r['network_rows'] / full_rows:.4f} | " + ("-" if name == "a" else f"{r['psnr_vs_a']:.2f} dB") + " |")
        say()
        say(f"Time against rows: (b) / (a) = {rows['b']['median_s'] / rows['a']['median_s']:.4f} of the time for "
            f"{rows['b']['network_rows'] / full_rows:.4f} of the rows; (c) / (a) = {rows['c']['median_s'] / rows['a']['median_s']:.4f} for "
            f"{rows['c']['network_rows'] / full_rows:.4f}; (c1) / (b1) = {rows['c1']['median_s'] / rows['b1']['median_s']:.4f} for the same rows "
            f"(the rows kernel + the lost MotionNet reuse).")
        if bias is None and args.baseline:
            for path in args.baseline:
                with open(path) as f:
                    b = json.load(f)
                say(f"(a) of the checkout `{b['tree']}` in a process of its own, same session (`{b['command']}`): median {b['a_median_s']:.3f} s, "
                    f"{min(b['a_s']):.3f} .. {max(b['a_s']):.3f}; this checkout's (a) is x{rows['a']['median_s'] / b['a_median_s']:.4f} of it.")
            result["baseline"] = [json.load(open(path)) for path in args.baseline]
        c_tested, c_skipped = coarse_samples(model, built["c"])
        t_all, k_all = rows["c"]["samples_tested"], rows["c"]["samples_skipped"]
        say(f"(c) per stage: coarse {c_tested} tested / {c_skipped} skipped ({100 * c_skipped / max(c_tested, 1):.1f} %), "
            f"fine {t_all - c_tested} / {k_all - c_skipped} ({100 * (k_all - c_skipped) / max(t_all - c_tested, 1):.1f} %).")
        # the rows launches of one (c) frame, timed by the library's profiler
        model.set_occupancy(built["c"])
        built["c"].reset_stats()
        ops.profile_begin()
        parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        recs = ops.profile_end()
        model.set_occupancy(None)
        s = built["c"].stats()["samples"]
        tested, skipped = sum(t for t, _ in s.values()), sum(k for _, k in s.values())
        rk = [r for r in recs if r["kernel"] == "occupancy_rows"]
        rows_ms, all_ms = sum(r["ms"] for r in rk), sum(r["ms"] for r in recs)
        rows_bytes = 12 * tested + 16 * skipped + 4 * (tested - skipped)
        say(f"Rows launches of one (c) frame: {len(rk)} launches, {rows_ms:.3f} ms of {all_ms:.1f} ms launch time ({100 * rows_ms / all_ms:.3f} %); "
            f"{rows_bytes / 1e9:.3f} GB (12 B read per tested sample, 16 B written per skipped one, 4 B per listed one) = "
            f"{rows_bytes / 1e9 / max(rows_ms / 1e3, 1e-9):.0f} GB/s.")
        say()
        result[tag] = dict(noise_psnr=noise, variants=rows, full_rows=full_rows, coarse_tested=c_tested, coarse_skipped=c_skipped,
                           rows_ms=rows_ms, launch_ms=all_ms, rows_GB=rows_bytes / 1e9)
        del model
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
