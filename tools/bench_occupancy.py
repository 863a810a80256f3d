"""A/B of the occupancy grids (stnerf_amd.OccupancyGrids) on a bench.py workload's frame.

    python tools/bench_occupancy.py [--workload taekwondo-1080p-64+64] [--reps 3] [--sparse-bias -3.0] [--no-sweep] [--md out.md]
    python tools/bench_occupancy.py --tree DIR --legs plain --json parent.json     # variant (a) alone, of ANOTHER checkout (built in place)
    rocprofv3 --kernel-trace --stats -d DIR -o occ --output-format csv -- python tools/bench_occupancy.py --legs trace
                                                                                   # one (a), (d), (b), (d) frame each: the cull kernel's own time
    python tools/bench_occupancy.py --baseline parent.json [parent2.json ...] ...  # ... and its frame time next to this checkout's (a)

One camera, one frame, rendered in one process under these variants, interleaved, `--reps` repetitions each after a warm-up:
  (a) occupancy off;
  (b) all-ones manual grids (the cull runs and culls nothing: its overhead);
  (c) manual grids that are the ellipsoid inscribed in each performer's box (pi / 6 = 52.4 % of the box's volume), 64 cells a side;
  (d) grids built from the model's own densities with OccupancyGrids' defaults,
on the bench scene and (a, d) on a SPARSE variant of it: the same scene with `synthetic.make_state_dict(sigma_bias=...)`, negative
enough that the stated share of the grid vertices is empty.  Then, for (d) on both scenes, a sweep of res {32, 64, 128} x dilate
{0, 1, 2}, one frame each.  Reported: frame times, pairs tested and culled per layer, build time per grid, the PSNR of every culled
frame against (a) on the same draws, the PSNR of (a) against itself under another seed (the render's own jitter noise), and the
cull launches' time and bytes per second from the library's launch profiler.  `--legs plain` renders only (a) on the bench scene,
through nothing the occupancy feature added, so that it also runs on the parent commit's checkout (`--tree`); run it in the same
session, before and after the main run, and hand its records to `--baseline`.  The sparse scene is another frame than the bench
scene, not the same frame with thinner performers: `make_state_dict(sigma_bias=...)` lowers the bias of the BACKGROUND's density
heads too, so its (a) is compared with its own (d) only.  Prints a markdown report (also to --md) and ONE JSON line.  The fields are synthetic random fields, not people: see profiles/occupancy_ab.md for what that does and does not show.
"""
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
    ap.add_argument("--tree", default=REPO, help="checkout to measure (default: this one)")
    ap.add_argument("--legs", default="all", choices=["all", "plain", "trace"],
                    help="plain: variant (a) on the bench scene only; trace: three culled frames for a kernel trace")
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    ap.add_argument("--baseline", nargs="*", default=[], help="records of --legs plain runs of the parent commit, same session")
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--sparse-bias", type=float, default=-3.0, help="sigma_bias of the sparse scene's density heads (the bench scene: 0.5)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    if args.legs != "plain":
        from stnerf_amd.occupancy import OccupancyGrids, box_bounds
    if not torch.cuda.is_available():
        sys.exit("bench_occupancy.py needs an MI355X (the render path has no CPU fallback)")
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
        if grids is not None:
            model.set_occupancy(grids)
        model.seed = seed
        if grids is not None:
            grids.reset_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        if grids is not None:
            model.set_occupancy(None)
        return dt_s, out[0][0], (grids.stats() if grids is not None else None)

    def manual(model, occupied):
        g = OccupancyGrids(auto=False)
        for i in range(1, L + 1):
            g.set_manual(i, occupied, *box_bounds(model.layer_box_at(i, ids[i])))
        return g

    def empty_share(model, res=64):
        out = {}
        for i in range(1, L + 1):
            dense = None
            for fine in (False, True):
                s, _, _ = model.density_grid(i, ids[i], res, fine=fine)
                d = ~(s <= 1e-4)
                dense = d if dense is None else dense | d
            out[i] = 1.0 - float(dense.float().mean())
        return out

    def build_ms(model, grids):
        """Milliseconds per grid of a fresh build (the networks at the vertices + the bit table)."""
        grids.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(1, L + 1):
            grids.grid(model, i, ids[i], device)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / L

    def occupied_share(model, grids):
        out = {}
        for i in range(1, L + 1):
            g = grids.grid(model, i, ids[i], device)
            bits = g.bits.cpu().numpy().view(np.uint32)
            out[i] = float(sum(bin(int(w)).count("1") for w in bits)) / (g.res[0] * g.res[1] * g.res[2])
        return out

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frame_ids=ids,
                             tree=os.path.basename(os.path.abspath(args.tree)), command=" ".join(["python", "tools/bench_occupancy.py"] + sys.argv[1:]))
    if args.legs == "plain":
        model = scene()
        frame(model, None)
        frame(model, None)                                              # the same two warm-up frames as the main run
        result["a_s"] = [frame(model, None)[0] for _ in range(args.reps)]
        result["a_median_s"] = statistics.median(result["a_s"])
        if args.json:
            with open(args.json, "w") as f:
                json.dump(result, f)
        print(json.dumps(result))
        return
    if args.legs == "trace":
        model = scene()
        auto = OccupancyGrids()
        result["frames"] = []
        for name, grids in (("a", None), ("d", auto), ("b", manual(model, torch.ones(8, 8, 8, dtype=torch.bool))), ("d", auto)):
            t, _, st_ = frame(model, grids)
            pairs = (st_ or {}).get("pairs", {})
            result["frames"].append(dict(variant=name, frame_s=t, tested=sum(x for x, _ in pairs.values()), culled=sum(c for _, c in pairs.values())))
        result["tested_pairs_total"] = sum(f["tested"] for f in result["frames"])
        result["cull_point_bytes_total"] = 12 * n1 * result["tested_pairs_total"]
        print(json.dumps(result))
        return
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}, performer frame ids {ids[1:]}.")
    say()
    for tag, bias in (("bench scene", None), ("sparse scene (sigma_bias %.1f)" % args.sparse_bias, args.sparse_bias)):
        model = scene(bias)
        variants = [("a", lambda: None)]
        if bias is None:
            variants += [("b", lambda: manual(model, torch.ones(8, 8, 8, dtype=torch.bool))), ("c", lambda: manual(model, ellipsoid(64)))]
        auto = OccupancyGrids()
        variants.append(("d", lambda: auto))
        built = {name: make() for name, make in variants}
        share = empty_share(model)
        frame(model, None)                                              # warm-up: packs, workspace, clocks
        frame(model, auto)                                              # ... and the grids of (d)
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
        say(f"Share of the 65^3 grid vertices that are empty (sigma <= 1e-4 in both networks), per performer: "
            + ", ".join(f"layer {i}: {100 * s:.1f} %" for i, s in share.items()) + ".")
        say(f"PSNR of (a) against (a) under another seed (the render's own jitter noise): {noise:.2f} dB.")
        say()
        say("| variant | frame s (median) | min .. max | vs (a) | pairs tested / culled per layer | culled share | PSNR vs (a) |")
        say("|---|---|---|---|---|---|---|")
        rows = {}
        for name in built:
            med = statistics.median(times[name])
            pairs = (stats[name] or {}).get("pairs", {})
            tested, culled = sum(t for t, _ in pairs.values()), sum(c for _, c in pairs.values())
            rows[name] = dict(median_s=med, min_s=min(times[name]), max_s=max(times[name]), pairs={str(k): v for k, v in pairs.items()},
                              culled_share=culled / tested if tested else None,
                              psnr_vs_a=None if name == "a" else psnr(images[name], images["a"]))
            say(f"| ({name}) | {med:.3f} | {min(times[name]):.3f} .. {max(times[name]):.3f} | x{statistics.median(times['a']) / med:.3f} | "
                + (", ".join(f"{i}: {t} / {c}" for i, (t, c) in pairs.items()) or "-") + " | "
                + (f"{100 * culled / tested:.1f} %" if tested else "-") + " | "
                + ("-" if name == "a" else f"{rows[name]['psnr_vs_a']:.2f} dB") + " |")
        if bias is None and args.baseline:
            a_med = statistics.median(times["a"])
            for path in args.baseline:
                with open(path) as f:
                    b = json.load(f)
                say(f"(a) of the checkout `{b['tree']}` in a process of its own, same session (`{b['command']}`): median {b['a_median_s']:.3f} s, "
                    f"{min(b['a_s']):.3f} .. {max(b['a_s']):.3f}; this checkout's (a) is x{a_med / b['a_median_s']:.4f} of it.")
            result["baseline"] = [json.load(open(path)) for path in args.baseline]
        say()
        bms = build_ms(model, auto)
        occ_share = occupied_share(model, auto)
        say(f"(d): res {auto.res}, threshold {auto.threshold}, dilate {auto.dilate}; build {bms:.1f} ms per grid; occupied cells: "
            + ", ".join(f"layer {i}: {100 * s:.1f} %" for i, s in occ_share.items()) + ".")
        # the cull launches of one (d) frame, timed by the library's profiler
        model.set_occupancy(auto)
        auto.reset_stats()
        ops.profile_begin()
        parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        recs = ops.profile_end()
        model.set_occupancy(None)
        cull = [r for r in recs if r["kernel"] == "occupancy_cull"]
        cull_ms, all_ms = sum(r["ms"] for r in cull), sum(r["ms"] for r in recs)
        tested = sum(t for t, _ in auto.stats()["pairs"].values())
        cull_bytes = 12 * n1 * tested + sum(r["n_rays"] for r in cull)
        say(f"Cull launches of one (d) frame: {len(cull)} launches, {cull_ms:.3f} ms of {all_ms:.1f} ms launch time "
            f"({100 * cull_ms / all_ms:.3f} %); {cull_bytes / 1e9:.3f} GB (12 n1 bytes per tested pair + one mask byte per ray and launch) "
            f"= {cull_bytes / 1e9 / (cull_ms / 1e3):.0f} GB/s.")
        say()
        result[tag] = dict(empty_vertex_share={str(k): v for k, v in share.items()}, noise_psnr=noise, variants=rows, build_ms_per_grid=bms,
                           occupied_share={str(k): v for k, v in occ_share.items()}, cull_ms=cull_ms, launch_ms=all_ms, cull_GB=cull_bytes / 1e9)
        if not args.no_sweep:
            say("| res | dilate | frame s | vs (a) | culled share | PSNR vs (a) | build ms / grid |")
            say("|---|---|---|---|---|---|---|")
            sweep = []
            for res in (32, 64, 128):
                for dil in (0, 1, 2):
                    g = OccupancyGrids(res=res, dilate=dil)
                    model.set_occupancy(None)
                    b = build_ms(model, g)
                    t, img, st_ = frame(model, g)
                    tested, culled = sum(x for x, _ in st_["pairs"].values()), sum(c for _, c in st_["pairs"].values())
                    p = psnr(img, images["a"])
                    sweep.append(dict(res=res, dilate=dil, frame_s=t, culled_share=culled / max(tested, 1), psnr_vs_a=p, build_ms_per_grid=b))
                    say(f"| {res} | {dil} | {t:.3f} | x{statistics.median(times['a']) / t:.3f} | {100 * culled / max(tested, 1):.1f} % | {p:.2f} dB | {b:.1f} |")
            say()
            ok = [r for r in sweep if r["psnr_vs_a"] >= noise]
            best = min(ok, key=lambda r: r["frame_s"]) if ok else None
            say(f"Pairs whose PSNR against (a) is not below the jitter noise ({noise:.2f} dB): "
                + (", ".join(f"{r['res']}/{r['dilate']}" for r in ok) or "none") + "; the cheapest of them by frame time: "
                + (f"res {best['res']}, dilate {best['dilate']}" if best else "-") + ".")
            say()
            result[tag]["sweep"] = sweep
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
