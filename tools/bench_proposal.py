"""A/B of the grid proposals (stnerf_amd.ProposalGrids) on a bench.py workload's frame.

    python tools/bench_proposal.py [--workload taekwondo-1080p-64+64] [--reps 3] [--res 64 128 256] [--md out.md] [--json out.json]

One camera, one frame, rendered in one process under three legs, interleaved, `--reps` repetitions each after a warm-up, for every
`--res`:
  (a) exact: no proposal;
  (b) the performers flagged: their coarse densities come from grids of `res` cells a side, their coarse networks do not run;
  (c) the performers and the background flagged.
Reported per leg: frame time (median, min .. max), the time of a fresh build of its grids and the device bytes they take, and the PSNR
of the fine mixed colour against (a) at the same seed.  Next to that PSNR stands the yardstick: (a) against itself under another seed,
the render's own sampling noise.  Prints a markdown report (also to --md) and ONE JSON line.  The fields are synthetic random fields
(a fog), not surfaces: see profiles/proposal_ab.md for what that does and does not show.
"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--res", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.proposal import ProposalGrids
    if not torch.cuda.is_available():
        sys.exit("bench_proposal.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [1.0 + (0.5 * i + 0.25) % 2 for i in range(L)]           # fractional performer frame ids
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.seed, model.fresh_draws_per_call = 0, False

    def frame(grids, seed=0):
        model.set_proposal(grids)
        model.seed = seed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        model.set_proposal(None)
        return dt_s, out[0][0]

    def build(grids):
        """(milliseconds of a fresh build of every grid the leg uses, the bytes they take)."""
        grids.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in grids.flagged_layers(model):
            grids.grid(model, i, ids[i], device)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), grids.stats()["bytes"]

    lines = []
    result = dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frame_ids=ids,
                  command=" ".join(["python", "tools/bench_proposal.py"] + sys.argv[1:]), legs=[])
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}, performer frame ids {ids[1:]}.")
    say()
    frame(None)                                                         # warm-up: packs, workspace, clocks
    frame(None)
    _, exact = frame(None)
    _, other_seed = frame(None, seed=1)
    noise = psnr(other_seed, exact)
    result["noise_psnr"] = noise
    say(f"Yardstick: PSNR of (a) against (a) under another seed (the render's own sampling noise): {noise:.2f} dB.")
    say()
    say("| res | leg | frame ms (median) | min .. max | vs (a) | grid build ms | grid bytes | PSNR vs (a), same seed |")
    say("|---|---|---|---|---|---|---|---|")
    for res in args.res:
        legs = [("a", None), ("b", ProposalGrids(res=res, max_grids=64)), ("c", ProposalGrids(res=res, background=True, max_grids=64))]
        builds = {name: ((0.0, 0) if g is None else build(g)) for name, g in legs}
        for name, g in legs:
            frame(g)                                                    # the grids of the leg, and its launches once
        times, images = {name: [] for name, _ in legs}, {}
        for _ in range(args.reps):
            for name, g in legs:
                t, images[name] = frame(g)
                times[name].append(1e3 * t)
        a_med = statistics.median(times["a"])
        for name, g in legs:
            med = statistics.median(times[name])
            rec = dict(res=res, leg=name, median_ms=med, min_ms=min(times[name]), max_ms=max(times[name]), build_ms=builds[name][0],
                       grid_bytes=builds[name][1], psnr_vs_a=None if name == "a" else psnr(images[name], images["a"]))
            result["legs"].append(rec)
            say(f"| {res} | ({name}) | {med:.1f} | {rec['min_ms']:.1f} .. {rec['max_ms']:.1f} | x{a_med / med:.3f} | "
                + ("-" if g is None else f"{rec['build_ms']:.1f}") + " | " + ("-" if g is None else f"{rec['grid_bytes'] / 1e6:.1f} MB") + " | "
                + ("-" if name == "a" else f"{rec['psnr_vs_a']:.2f} dB") + " |")
        del legs
        torch.cuda.empty_cache()
    say()
    # the lookup launches of one (b) frame at the last res, timed by the library's profiler
    g = ProposalGrids(res=args.res[-1], max_grids=64)
    frame(g)
    model.set_proposal(g)
    ops.profile_begin()
    parallel.render_view(model, K, T, H, W, ids, device=device)
    torch.cuda.synchronize()
    recs = ops.profile_end()
    model.set_proposal(None)
    look = [r for r in recs if r["kernel"] == "proposal_density"]
    look_ms, all_ms = sum(r["ms"] for r in look), sum(r["ms"] for r in recs)
    result.update(lookup_ms=look_ms, launch_ms=all_ms, lookup_launches=len(look))
    say(f"Lookup launches of one (b) frame at res {args.res[-1]}: {len(look)} launches, {look_ms:.3f} ms of {all_ms:.1f} ms launch time "
        f"({100 * look_ms / max(all_ms, 1e-9):.2f} %).")
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
