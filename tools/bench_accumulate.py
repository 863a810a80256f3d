"""Progressive multi-sample frames (stnerf_amd.accumulate) on a bench.py workload's frame: what the passes
cost and what they buy.

    python tools/bench_accumulate.py [--workload taekwondo-1080p-64+64] [--tols auto | t1,t2,t3] [--ref-spp 32] [--md out.md]

One camera, one frame (bench.py's first step: orbit 10 degrees, frame ids 1 / 2.5, thresholds 0), rendered in one process as
  fixed 1 spp, fixed 8 spp, and adaptive (min 2, max 8) at three values of tol
(``--tols auto``: the 25 %, 50 % and 75 % quantiles over the pixels of the standard error of the mean after two passes, so that about
three quarters, half and a quarter of the pixels go on after the second pass).  For each: seconds, rays rendered, the histogram of
samples per pixel, and the PSNR of the mixed colour against a ``--ref-spp`` frame rendered under OTHER seeds (it shares no sample
with the frames it judges).  Then the accumulate and select launches alone, timed with device events on the frame's own state, next
to the bytes the accumulator must move ((3 C + 2 V + 2) floats per pixel per pass).  Reported, not asserted: the scene is a dense
synthetic random field, and how quickly real footage converges nobody has measured.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--tols", default="auto", help="three tolerances t1,t2,t3, or auto: quantiles of the standard error after two passes")
    ap.add_argument("--max-spp", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=32)
    ap.add_argument("--shutter", type=float, default=0.0, help="exposure of the performers in frames (0: anti-aliasing and noise only)")
    ap.add_argument("--launches-only", action="store_true", help="skip the frames: time the accumulate and select launches alone")
    ap.add_argument("--md", default=None, help="also write the markdown report to this file")
    ap.add_argument("--json", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import bench                                                        # the workload table and the scene builder of the flagship benchmark
    from stnerf_amd import ops, parallel, synthetic as syn
    from stnerf_amd.accumulate import AccumulateSpec
    if not torch.cuda.is_available():
        sys.exit("bench_accumulate.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    H, W, L, n1, n2, st, dt = bench.WORKLOADS[args.workload]
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    ids = [1.0] + [2.5] * L
    model, _ = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.fresh_draws_per_call = False
    shutter = dict(shutter=args.shutter, frame_range=(1.0, 3.0)) if args.shutter else {}

    def frame(spec, seed=0):
        model.seed = seed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, stats = parallel.render_view_accumulated(model, K, T, H, W, ids, spec, device=device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out[0][0], stats

    lines, result = [], dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1,
                             command=" ".join(["python", "tools/bench_accumulate.py"] + sys.argv[1:]))
    say = lambda s="": (lines.append(s), print(s, flush=True))
    say(f"## `{result['command']}`")
    say()
    say(f"{args.workload}: {H * W} rays, {n1}+{n2} samples, {L} performers, {args.precision}; pixel filter 1.0, shutter {args.shutter}.")
    say()
    if not args.launches_only:
        result.update(frames_of(args, say, frame, model, parallel, AccumulateSpec, K, T, H, W, ids, shutter, device))
    result.update(launches_of(say, ops, H, W, L + 1, result.get("tols", [0.0, 2e-3])[1], result.get("pass_s"), device))
    if args.md:
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f)
    print(json.dumps(result))


def frames_of(args, say, frame, model, parallel, AccumulateSpec, K, T, H, W, ids, shutter, device):
    """The frames: fixed 1 spp, fixed max spp, adaptive at three tolerances, each against the reference frame."""
    frame(AccumulateSpec(1))                                            # warm-up: packs, workspace, clocks
    t_plain0 = time.perf_counter()
    model.seed = 0
    plain = parallel.render_view(model, K, T, H, W, ids, device=device)
    torch.cuda.synchronize()
    t_plain = time.perf_counter() - t_plain0
    _, two, two_stats = frame(AccumulateSpec(2, **shutter))
    se = two_stats["variance"].max(1)[0].sqrt()
    if args.tols == "auto":
        tols = [float(torch.quantile(se, q)) for q in (0.25, 0.5, 0.75)]
    else:
        tols = [float(x) for x in args.tols.split(",")]
    t_ref, ref, ref_stats = frame(AccumulateSpec(args.ref_spp, **shutter), seed=1000)
    legs = [("fixed 1 spp", AccumulateSpec(1, **shutter)), (f"fixed {args.max_spp} spp", AccumulateSpec(args.max_spp, **shutter))]
    legs += [(f"adaptive (2, {args.max_spp}), tol {t:.3e}", AccumulateSpec(args.max_spp, 2, t, **shutter)) for t in tols]
    say(f"`render_view` of the same frame (no accumulation): {t_plain:.3f} s.  Reference: {args.ref_spp} spp under seeds 1000.., {t_ref:.1f} s.  "
        f"Standard error of the mean after two passes (largest colour channel): quartiles "
        + " / ".join(f"{float(torch.quantile(se, q)):.3e}" for q in (0.25, 0.5, 0.75)) + ".")
    say()
    say("| frame | seconds | passes | rays rendered | x of one pass | spp histogram (spp: pixels) | PSNR vs the reference |")
    say("|---|---|---|---|---|---|---|")
    rows = []
    for name, spec in legs:
        t, img, stats = frame(spec)
        hist = torch.bincount(stats["spp"].to(torch.int64)).tolist()
        row = dict(frame=name, seconds=t, passes=stats["passes"], rays_rendered=stats["rays_rendered"],
                   spp_histogram={str(k): v for k, v in enumerate(hist) if v}, psnr_vs_reference=psnr(img, ref),
                   mean_spp=stats["rays_rendered"] / (H * W))
        rows.append(row)
        say(f"| {name} | {t:.3f} | {row['passes']} | {row['rays_rendered']} | {row['mean_spp']:.3f} | "
            + ", ".join(f"{k}: {v}" for k, v in row["spp_histogram"].items()) + f" | {row['psnr_vs_reference']:.2f} dB |")
    say()
    again = frame(AccumulateSpec(1, **shutter))[1]
    say(f"The 1-spp frame equals `render_view` of the frame bit for bit: {bool(torch.equal(plain[0][0], again))} (pass 0 is the plain render).")
    say()
    return dict(render_view_s=t_plain, reference=dict(spp=args.ref_spp, seconds=t_ref), tols=tols, frames=rows, pass_s=rows[0]["seconds"])


def launches_of(say, ops, H, W, l, tol, pass_s, device):
    """The accumulate and select launches alone, on a state as large as the frame's: fresh values every pass (so that m2 > 0 and
    the select has a list to write), timed between device events."""
    Cw = 5 + 5 * l
    values = [torch.rand(H * W, Cw + 1, device=device)[:, :Cw] for _ in range(4)]     # (the row stride of the packed outputs)
    state = ops.accumulate_state(H * W, Cw, 3, device)
    for i in range(3):
        ops.accumulate(values[i], state)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc_ms, sel_ms, sel_wall = [], [], []
    for i in range(10):
        a, b = ev(), ev()
        a.record()
        ops.accumulate(values[i % 4], state)
        b.record()
        torch.cuda.synchronize()
        acc_ms.append(a.elapsed_time(b))
    n_sel = 0
    for _ in range(10):
        a, b = ev(), ev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        _, n_sel = ops.accumulate_select(state, 2, 1 << 14, tol)
        b.record()
        torch.cuda.synchronize()
        sel_wall.append((time.perf_counter() - t0) * 1e3)
        sel_ms.append(a.elapsed_time(b))
    acc_bytes = (3 * Cw + 2 * 3 + 2) * 4 * H * W
    sel_bytes = 2 * (3 + 1) * 4 * H * W + 2 * 4 * n_sel
    am, sm = statistics.median(acc_ms), statistics.median(sel_ms)
    say(f"Accumulate alone (C = {Cw}, V = 3, {H * W} rows, no list; two launches): median {am:.3f} ms of 10 ({min(acc_ms):.3f} .. {max(acc_ms):.3f}); "
        f"derived traffic (3 C + 2 V + 2) x 4 B per pixel = {acc_bytes / 1e9:.3f} GB -> {acc_bytes / 1e9 / (am / 1e3):.0f} GB/s.")
    say(f"Select alone (tol {tol:.3e}: {n_sel} of {H * W} pixels active; three launches, the copy of the list and one D2H): median {sm:.3f} ms of 10 "
        f"between device events ({min(sel_ms):.3f} .. {max(sel_ms):.3f}), {statistics.median(sel_wall):.3f} ms on the host clock with the read-back; it "
        f"reads m2 and count twice, writes the list and copies it: {sel_bytes / 1e9:.3f} GB.")
    if pass_s:
        say(f"Against a pass: accumulate + select = {(am + sm) / 1e3:.4f} s of the {pass_s:.3f} s a whole-view pass takes "
            f"({100 * (am + sm) / 1e3 / pass_s:.3f} %).")
    return dict(accumulate_ms=acc_ms, select_ms=sel_ms, select_wall_ms=sel_wall, accumulate_GB=acc_bytes / 1e9, select_GB=sel_bytes / 1e9,
                select_active=n_sel)


if __name__ == "__main__":
    main()
