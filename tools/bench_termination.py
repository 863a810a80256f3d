"""A/B of early ray termination (model.set_termination) on a bench.py workload's frame.

    python tools/bench_termination.py [--workload taekwondo-1080p-64+64] [--reps 3] [--tau 1e-4] [--md out.md] [--json out.json]
    python tools/bench_occupancy.py --tree DIR --legs plain --json parent.json     # variant (a) alone, of the parent commit's checkout
    python tools/bench_termination.py --baseline parent.json [parent2.json ...]    # ... its frame time next to this checkout's (a)

The method and the scene are tools/bench_sample_cull.py's: one camera, one frame, rendered in one process under the variants below,
interleaved, `--reps` repetitions each after warm-up frames; the grids of (c) / (ct) are the manual ellipsoid inscribed in each
performer's box, 64 cells a side, ray cull + sample cull:
  (a)   no termination, no grids;
  (a0)  (a) with STNERF_MOTION_REUSE=0: every performer's MotionNet fused -- what the reuse a terminated performer gives up is worth;
  (t)   termination alone: every layer and the background, tau = --tau;
  (tp)  termination with the background flag off (performers only);
  (c)   ray cull + sample cull;
  (ct)  (c) + termination (every layer and the background).
Reported: frame times; per terminated layer the fine rows tested and listed, from the counters; PSNR and maximum absolute difference
of the fine mixed colour against the un-terminated counterpart ((t), (tp) against (a); (ct) against (c)) on the same draws; the same at
tau = 1e-4, 1e-3, 1e-2; and, from the library's launch profiler, the time of the ray_stop and visibility_rows launches and of the
compositor with and without the merged-weights output.  Prints a markdown report (also to --md) and ONE JSON line.  The fields are
synthetic random fields, not people: what is hidden here says nothing about a captured scene."""
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
    ap.add_argument("--tau", type=float, default=1e-4)
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.occupancy import OccupancyGrids, box_bounds
    from stnerf_amd.termination import Termination
    if not torch.cuda.is_available():
        sys.exit("bench_termination.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [1.0 + (0.5 * i + 0.25) % 2 for i in range(L)]           # fractional performer frame ids
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.seed, model.fresh_draws_per_call = 0, False
    grids = OccupancyGrids(auto=False, samples=True)
    for i in range(1, L + 1):
        grids.set_manual(i, ellipsoid(64), *box_bounds(model.layer_box_at(i, ids[i])))

    def frame(term=None, occ=None, reuse=True, profile=False):
        """-> (seconds, fine mixed colour, termination rows {layer: (tested, not listed)}, launch records | None)"""
        model.set_occupancy(occ)
        model.set_termination(term)
        model.seed = 0
        if reuse:
            os.environ.pop("STNERF_MOTION_REUSE", None)
        else:
            os.environ["STNERF_MOTION_REUSE"] = "0"
        for s in (term, occ):
            if s is not None:
                s.reset_stats()
        torch.cuda.synchronize()
        if profile:
            ops.profile_begin()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        recs = ops.profile_end() if profile else None
        rows = term.stats()["rows"] if term is not None else {}
        model.set_occupancy(None)
        model.set_termination(None)
        os.environ.pop("STNERF_MOTION_REUSE", None)
        return dt_s, out[0][0], rows, recs

    variants = {"a": dict(), "a0": dict(reuse=False), "t": dict(term=Termination(args.tau)), "tp": dict(term=Termination(args.tau, background=False)),
                "c": dict(occ=grids), "ct": dict(term=Termination(args.tau), occ=grids)}
    against = {"a0": "a", "t": "a", "tp": "a", "ct": "c"}
    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frame_ids=ids, tau=args.tau,
                             command=" ".join(["python", "tools/bench_termination.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}, performer frame ids {ids[1:]}, tau {args.tau:g}; "
        f"grids of (c) / (ct): the ellipsoid inscribed in each box, 64 cells a side, ray cull + sample cull.")
    say()
    frame()                                                             # warm-up: packs, workspace, clocks
    frame(**variants["ct"])                                             # ... and the largest workspace
    times, rows, images = {k: [] for k in variants}, {}, {}
    for _ in range(args.reps):
        for name, kw in variants.items():
            t, img, rw, _ = frame(**kw)
            times[name].append(t)
            rows[name], images[name] = rw, img
    say("| variant | frame s (median) | min .. max | vs its un-terminated counterpart | fine rows tested / listed per layer | PSNR | max abs diff |")
    say("|---|---|---|---|---|---|---|")
    table = {}
    for name in variants:
        med = statistics.median(times[name])
        ref = against.get(name)
        r = dict(median_s=med, min_s=min(times[name]), max_s=max(times[name]), rows={str(i): [t, t - k] for i, (t, k) in rows[name].items()})
        if ref is not None:
            r["vs"] = statistics.median(times[ref]) / med
            r["psnr"] = psnr(images[name], images[ref])
            r["max_abs"] = float((images[name] - images[ref]).abs().max())
        table[name] = r
        per_layer = ", ".join(f"{i}: {t} / {t - k} ({100 * (t - k) / max(t, 1):.1f} %)" for i, (t, k) in rows[name].items()) or "-"
        say(f"| ({name}) | {med:.3f} | {r['min_s']:.3f} .. {r['max_s']:.3f} | " + (f"x{r['vs']:.3f} vs ({ref})" if ref else "-") + f" | {per_layer} | "
            + (f"{r['psnr']:.2f} dB" if ref else "-") + " | " + (f"{r['max_abs']:.3e}" if ref else "-") + " |")
    say()
    result["variants"] = table
    if args.baseline:
        result["baseline"] = []
        for path in args.baseline:
            with open(path) as f:
                b = json.load(f)
            result["baseline"].append(b)
            say(f"(a) of the checkout `{b['tree']}` in a process of its own, same session (`{b['command']}`): median {b['a_median_s']:.3f} s, "
                f"{min(b['a_s']):.3f} .. {max(b['a_s']):.3f}; this checkout's (a) is x{table['a']['median_s'] / b['a_median_s']:.4f} of it.")
        say()
    # the picture at three tau (measured, not asserted: the coarse stop depth bounds what the COARSE networks saw)
    say("| tau | frame s | fine rows tested / listed, all layers | PSNR vs (a) | max abs diff vs (a) |")
    say("|---|---|---|---|---|")
    sweep = {}
    for tau in (1e-4, 1e-3, 1e-2):
        t, img, rw, _ = frame(term=Termination(tau))
        tested, skipped = sum(v[0] for v in rw.values()), sum(v[1] for v in rw.values())
        sweep[str(tau)] = dict(frame_s=t, tested=tested, listed=tested - skipped, psnr=psnr(img, images["a"]), max_abs=float((img - images["a"]).abs().max()))
        say(f"| {tau:g} | {t:.3f} | {tested} / {tested - skipped} ({100 * (tested - skipped) / max(tested, 1):.1f} %) | {sweep[str(tau)]['psnr']:.2f} dB | "
            f"{sweep[str(tau)]['max_abs']:.3e} |")
    say()
    result["tau_sweep"] = sweep
    # the new launches of one (t) frame, and the compositor with and without the merged weights, by the library's profiler
    _, _, rw, rec_t = frame(term=Termination(args.tau), profile=True)
    _, _, _, rec_a = frame(profile=True)
    ms = lambda recs, kernel, pred=lambda r: True: sum(r["ms"] for r in recs if r["kernel"] == kernel and pred(r))
    stop_ms, vis_ms = ms(rec_t, "ray_stop"), ms(rec_t, "visibility_rows")
    coarse = lambda r: r["ns"] == n1
    comp_t, comp_a = ms(rec_t, "composite", coarse), ms(rec_a, "composite", coarse)
    all_t, all_a = sum(r["ms"] for r in rec_t), sum(r["ms"] for r in rec_a)
    tested, skipped = sum(v[0] for v in rw.values()), sum(v[1] for v in rw.values())
    stop_bytes = H * W * ((L + 1) * n1 * 8 + 4)
    vis_bytes = 4 * tested + 16 * skipped + 4 * (tested - skipped)
    say(f"Launches of one (t) frame ({all_t:.1f} ms of launch time; an (a) frame: {all_a:.1f} ms): ray_stop {stop_ms:.3f} ms "
        f"({len([r for r in rec_t if r['kernel'] == 'ray_stop'])} launches, at most {stop_bytes / 1e9:.3f} GB read = {stop_bytes / 1e9 / max(stop_ms / 1e3, 1e-9):.0f} GB/s if all of it "
        f"were read), visibility_rows {vis_ms:.3f} ms ({len([r for r in rec_t if r['kernel'] == 'visibility_rows'])} launches, {vis_bytes / 1e9:.3f} GB = "
        f"{vis_bytes / 1e9 / max(vis_ms / 1e3, 1e-9):.0f} GB/s); the coarse compositor {comp_t:.3f} ms with the merged weights against {comp_a:.3f} ms without "
        f"(+ {comp_t - comp_a:.3f} ms).  Together {100 * (stop_ms + vis_ms + comp_t - comp_a) / all_t:.3f} % of the frame.")
    say(f"MotionNet reuse: (a0) / (a) = {table['a0']['median_s'] / table['a']['median_s']:.4f} -- what every performer's reuse is worth on this frame, "
        f"the most a frame that terminates every performer can lose of it.")
    result["profile"] = dict(ray_stop_ms=stop_ms, visibility_rows_ms=vis_ms, composite_coarse_ms_t=comp_t, composite_coarse_ms_a=comp_a, launch_ms_t=all_t,
                             launch_ms_a=all_a, tested=tested, skipped=skipped)
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
