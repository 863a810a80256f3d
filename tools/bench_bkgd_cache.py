"""A/B of the background cache (stnerf_amd.BackgroundCache) on a fixed-view time sweep at a bench.py workload's shape.

    python tools/bench_bkgd_cache.py [--workload taekwondo-1080p-64+64] [--frames 5] [--warmup 1] [--precision bf16x3]

One camera, k frames whose performer frame ids change (st-nerf's "time sweep from a fixed view"), every frame rendered twice in the
same process, interleaved: cache detached, then attached (`parallel.render_view`, the function `render_pose` runs).  The first
cached frame captures, the others are served from the cache.  Prints the per-frame times, whether each cached frame equals its
uncached twin bit for bit, the cache's statistics, the copy launches' achieved GB/s (the library's launch profiler on one more
cached frame) and ONE JSON line with all of it.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402  (the workload table and the scene builder of the flagship benchmark)
import stnerf_amd  # noqa: E402
from stnerf_amd import ops, parallel, synthetic as syn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--frames", type=int, default=5, help="timed frames per leg (after the warm-up frames)")
    ap.add_argument("--warmup", type=int, default=1, help="untimed frames per leg; the first cached one is the capture frame")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--budget-gb", type=float, default=None, help="the cache's budget (default: BackgroundCache's)")
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_bkgd_cache.py needs an MI355X (the render path has no CPU fallback)")
    if args.warmup < 1:
        sys.exit("--warmup must be >= 1: the first cached frame captures")
    device = torch.device("cuda", torch.cuda.current_device())
    model, (H, W, L, n1, n2, st, dt) = bench.build_scene(args.workload, device)
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.seed = 0
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    cache = stnerf_amd.BackgroundCache(None if args.budget_gb is None else int(args.budget_gb * (1 << 30)))
    frames_in_scene = model.bboxes.shape[0]
    # performer i of frame k: a fractional frame id that moves through the scene's frames
    frame_ids = lambda k: [1.0] + [1.0 + (0.25 * k + 0.5 * i) % (frames_in_scene - 1) for i in range(L)]

    def frame(k, cached):
        model.set_background_cache(cache if cached else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, frame_ids(k), device=device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    rows = []
    for k in range(args.warmup + args.frames):
        t_off, out_off = frame(k, False)
        t_on, out_on = frame(k, True)
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out_off[0], out_on[0]))
        kind = "capture" if k == 0 else ("warmup" if k < args.warmup else "timed")
        rows.append(dict(frame=k, kind=kind, off_s=t_off, on_s=t_on, bit_equal=bool(same)))
        print(f"frame {k:2d} ({kind:7s}) performer ids {frame_ids(k)[1:]}: cache off {t_off:7.3f} s   on {t_on:7.3f} s   "
              f"bit-equal {same}", flush=True)
        del out_off, out_on

    # the copy launches of one more cached frame, timed by the library's profiler (HIP events around each launch)
    model.set_background_cache(cache)
    ops.profile_begin()
    parallel.render_view(model, K, T, H, W, frame_ids(args.warmup + args.frames), device=device)
    torch.cuda.synchronize()
    recs = ops.profile_end()
    copies = [r for r in recs if r["kernel"] == "copy_layer_raw"]
    copy_bytes = sum(r["n_rays"] * r["bytes_per_ray"] for r in copies)
    copy_ms = sum(r["ms"] for r in copies)
    frame_ms = sum(r["ms"] for r in recs)
    model.set_background_cache(None)

    timed = [r for r in rows if r["kind"] == "timed"]
    off, on = [r["off_s"] for r in timed], [r["on_s"] for r in timed]
    result = dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=L + 1, frames=rows,
                  off_median_s=statistics.median(off), on_median_s=statistics.median(on),
                  off_min_max_s=[min(off), max(off)], on_min_max_s=[min(on), max(on)],
                  speedup=statistics.median(off) / statistics.median(on), all_bit_equal=all(r["bit_equal"] for r in rows),
                  cache_stats=dict(cache.stats), cache_bytes=cache.bytes_used, cache_pieces=len(cache),
                  copy_launches=len(copies), copy_GB=copy_bytes / 1e9, copy_ms=copy_ms,
                  copy_GBps=(copy_bytes / 1e9) / (copy_ms / 1e3) if copy_ms > 0 else None,
                  copy_share_of_launch_time=copy_ms / frame_ms if frame_ms > 0 else None)
    print(f"timed frames: cache off median {result['off_median_s']:.3f} s, on {result['on_median_s']:.3f} s "
          f"(x{result['speedup']:.2f}); cache {cache.stats}, {cache.bytes_used / 1e9:.2f} GB in {len(cache)} pieces")
    if copies:
        print(f"copy launches of a cached frame: {len(copies)} moving {result['copy_GB']:.2f} GB (read + write) in {copy_ms:.2f} ms "
              f"= {result['copy_GBps']:.0f} GB/s, {100 * result['copy_share_of_launch_time']:.2f} % of the frame's launch time")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
