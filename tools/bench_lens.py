"""The lens model in ray generation (stnerf_amd.lens): what the new ray generator costs beside the one it
extends, and what a frame through a lens costs beside a pinhole frame.

    python tools/bench_lens.py [--workload taekwondo-1080p-64+64] [--reps 20] [--spp 4] [--skip-frames] [--md profiles/lens_ab.md]

Rays: `stnerf_generate_rays_list` and `stnerf_generate_rays_lens` (distortion only, an aperture only, both) over the whole view of
the workload, no list, one frame-id column per layer; ``--reps`` launches each between device events after a warm-up launch, beside
the bytes a launch must write (24 + 4 columns per ray) and the 20 rounds' arithmetic.  Frames: `render_view` without and with a
distorting lens, and an accumulated frame of ``--spp`` passes without and with an aperture, one frame each after a warm-up frame.
Reported, not asserted.  Prints a markdown report (also to --md) and ONE JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COEFFS = dict(k1=-0.28, k2=0.09, k3=-0.01, p1=0.002, p2=0.001)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--focal", type=float, default=1500.0, help="focal length in pixels of the view the rays are generated for")
    ap.add_argument("--skip-frames", action="store_true", help="time the ray generators alone")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.accumulate import AccumulateSpec
    from stnerf_amd.lens import Lens
    if not torch.cuda.is_available():
        sys.exit("bench_lens.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=10.0)
    ids = [1.0] + [2.5] * L
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))
    result = dict(workload=args.workload, rays=H * W, command=" ".join(["python", "tools/bench_lens.py"] + sys.argv[1:]))
    say(f"## `{result['command']}`")
    say()

    # ---- the ray generators alone
    Kf = K.clone()
    Kf[0, 0] = Kf[1, 1] = args.focal
    focus = 4.0
    lenses = [("`stnerf_generate_rays_list` (no lens)", None),
              ("`stnerf_generate_rays_lens`, distortion only", Lens(**COEFFS)),
              ("`stnerf_generate_rays_lens`, an aperture only (phase 3 of 8, decorrelated)", Lens(aperture=0.05, focus=focus)),
              ("`stnerf_generate_rays_lens`, both", Lens(aperture=0.05, focus=focus, **COEFFS))]
    table = torch.from_numpy(Lens(aperture=0.05, focus=focus).table(8)).to(device)
    row_bytes = 4 * (6 + len(ids))
    say(f"Rays of the whole {H} x {W} view (f = {args.focal:g}), {len(ids)} frame-id columns: {row_bytes} B written per ray, "
        f"{row_bytes * H * W / 1e6:.1f} MB per launch; {args.reps} launches between device events after a warm-up launch.")
    say()
    say("| generator | ms, median (min .. max) | GB/s written |")
    say("|---|---|---|")
    rows = []
    for name, lens in lenses:
        kw = dict(offset=(0.25, 0.25))                                  # (a non-zero offset: the pixel-list entry without a lens)
        if lens is not None:
            kw.update(lens=lens, lens_phase=3, **(dict(lens_points=table) if lens.aperture > 0 else {}))
        ops.generate_rays(Kf, T, H, W, frame_ids=ids, device=device, **kw)
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            ops.generate_rays(Kf, T, H, W, frame_ids=ids, device=device, **kw)
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        rows.append(dict(generator=name, ms=ms, median_ms=med, GBps=row_bytes * H * W / 1e9 / (med / 1e3)))
        say(f"| {name} | {med:.4f} ({min(ms):.4f} .. {max(ms):.4f}) | {rows[-1]['GBps']:.0f} |")
    say()
    say("(Between the events lies the whole `ops.generate_rays` call: the output's allocation and the launch.  The 20 rounds are about "
        "400 flops and 40 quotient expansions per ray.)")
    say()
    result["generators"] = rows

    # ---- frames
    if not args.skip_frames:
        model, _ = bench.build_scene(args.workload, device)
        model.set_precision(args.precision)
        model.fresh_draws_per_call = False

        def timed(fn):
            model.seed = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        bend = Lens(k1=-0.1, k2=0.02, p1=0.001, p2=-0.0005)             # (mild: the workload's view has f = w, a wide one)
        deep = Lens(aperture=0.05, focus=focus)
        spec = AccumulateSpec(args.spp)
        timed(lambda: parallel.render_view(model, K, T, H, W, ids, device=device))      # warm-up: packs, workspace, clocks
        legs = [("`render_view`, no lens", lambda: parallel.render_view(model, K, T, H, W, ids, device=device)),
                ("`render_view`, distorting lens", lambda: parallel.render_view(model, K, T, H, W, ids, device=device, lens=bend)),
                (f"`render_view_accumulated`, {args.spp} spp, no lens", lambda: parallel.render_view_accumulated(model, K, T, H, W, ids, spec, device=device)),
                (f"`render_view_accumulated`, {args.spp} spp, aperture 0.05 focused at {focus:g}",
                 lambda: parallel.render_view_accumulated(model, K, T, H, W, ids, spec, device=device, lens=deep))]
        say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}; one frame per leg after a warm-up frame, seconds "
            "on the host clock around a device synchronise.")
        say()
        say("| frame | seconds |")
        say("|---|---|")
        frames = []
        for name, fn in legs:
            t, _ = timed(fn)
            frames.append(dict(frame=name, seconds=t))
            say(f"| {name} | {t:.3f} |")
        say()
        result["frames"] = frames
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
