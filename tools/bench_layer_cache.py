"""A/B of the layer cache (stnerf_amd.LayerCache) from a fixed view at a bench.py workload's shape.

    python tools/bench_layer_cache.py [--workload taekwondo-1080p-64+64] [--frames 4] [--precision bf16x3] [--out FILE.md]

One camera, three legs rendered in the same process -- no cache, the background cache alone, the background cache plus the layer
cache (`parallel.render_view`, the function `render_pose` runs) -- over three sweeps of --frames frames each:
  (a) a sweep of the LAST performer's shift (the other performers hold still: they are served from the cache);
  (b) a `layer_alpha` fade of performer 1 (nothing that feeds a network changes: no network runs);
  (c) a time sweep in which every performer's frame id changes every frame (nothing can be reused: the policy must make no capture
      after the second frame, and every frame is compared with the uncached one).
Every leg first renders the sweep's start state three times (sighting, capture, reuse), untimed.  Prints ms per frame (median and
range) per sweep and leg, whether the cached frames equal their uncached twins bit for bit, the bytes held per layer against the
dense figure, the listed copies' GB/s on algorithmic bytes (the library's launch profiler), ONE JSON line with all of it and, with
--out, the same as a markdown table.
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
from stnerf_amd.layer_cache import dense_bytes  # noqa: E402

LEGS = ("uncached", "background cache", "background + layer cache")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="taekwondo-1080p-64+64", choices=sorted(bench.WORKLOADS))
    ap.add_argument("--frames", type=int, default=4, help="timed frames per sweep and leg")
    ap.add_argument("--precision", default="bf16x3", choices=["fp32", "bf16x3"])
    ap.add_argument("--rays-per-launch", type=int, default=1 << 19)
    ap.add_argument("--orbit-deg", type=float, default=10.0)
    ap.add_argument("--out", default=None, help="also write the tables as markdown to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_layer_cache.py needs an MI355X (the render path has no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    model, (H, W, L, n1, n2, st, dt) = bench.build_scene(args.workload, device)
    if L < 2:
        sys.exit("bench_layer_cache.py needs a workload with two performers or more")
    model.max_rays_per_launch = args.rays_per_launch
    model.set_precision(args.precision)
    model.seed = 0
    l = L + 1
    K, T = syn.camera(H, W, orbit_deg=args.orbit_deg)
    frames_in_scene = model.bboxes.shape[0]
    still = [1.0] + [1.0 + 0.5 * i for i in range(L)]

    def state(sweep, k):
        """-> (frame ids, shift, layer_alpha) of frame k of a sweep; k = -1: the state of the untimed frames, which no timed frame
        repeats -- every timed frame of the shift sweep moves the last performer, none of the time sweep finds anything to reuse."""
        k = k if sweep == "time" else k + 1            # (shift / fade: the untimed frames hold step 0, timed frame k is step k + 1)
        shift = [[0.0, 0.0, 0.0] for _ in range(l)]
        alpha = [1.0] * l
        ids = list(still)
        if sweep == "shift":
            shift[L] = [0.02 * k, 0.0, 0.01 * k]
        elif sweep == "fade":
            alpha[1] = 1.0 - 0.15 * k
        else:
            ids = [1.0] + [1.0 + (0.25 * k + 0.5 * i) % (frames_in_scene - 1) for i in range(L)]
        return ids, shift, alpha

    def render(sweep, k):
        ids, shift, alpha = state(sweep, k)
        model.scale, model.shift, model.layer_alpha = [1.0] * l, shift, alpha
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = parallel.render_view(model, K, T, H, W, ids, device=device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def attach(leg, caches):
        model.set_background_cache(caches[0] if leg != "uncached" else None)
        model.set_layer_cache(caches[1] if leg == LEGS[2] else None)

    flat = lambda out: [t for part in (out[0], out[1], *out[2], *out[3]) for t in part] + list(out[4])
    result = dict(workload=args.workload, precision=args.precision, rays=H * W, n1=n1, n2=n2, layers=l, sweeps={})
    for sweep in ("shift", "fade", "time"):
        rows = {leg: [] for leg in LEGS}
        caches = (stnerf_amd.BackgroundCache(), stnerf_amd.LayerCache())
        same, captures_after_second = True, None
        for leg in LEGS:                                   # the start state three times: sighting, capture, reuse
            attach(leg, caches)
            for _ in range(3):
                render(sweep, -1)
        for k in range(args.frames):
            ref = None
            for leg in LEGS:                               # interleaved: the legs of a frame run back to back
                attach(leg, caches)
                before = caches[1].stats()["captures"]
                t, out = render(sweep, k)
                rows[leg].append(t)
                if leg == "uncached":
                    ref = flat(out)
                else:
                    same = same and all(torch.equal(a, b) for a, b in zip(flat(out), ref))
                if leg == LEGS[2] and sweep == "time" and k >= 2:
                    captures_after_second = (captures_after_second or 0) + caches[1].stats()["captures"] - before
                del out
        entry = dict(bit_equal=bool(same), layer_cache=caches[1].stats(mismatch=True), background_cache=dict(caches[0].stats))
        for leg in LEGS:
            ms = [1e3 * t for t in rows[leg]]
            entry[leg] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))
        if sweep == "time":
            entry["captures_after_second_frame"] = captures_after_second
            if captures_after_second:
                sys.exit(f"the time sweep captured {captures_after_second} entries after its second frame: the policy churns")
        # what the layer cache holds, per layer, against dense slices of the same pieces
        held = {}
        for key, capacity, nbytes, hits in caches[1].held():
            d = held.setdefault(key[0][1], dict(entries=0, hit_rays=0, bytes=0, dense_bytes=0))
            d["entries"] += 1
            d["hit_rays"] += capacity if hits is None else hits
            d["bytes"] += nbytes
            d["dense_bytes"] += dense_bytes(key[1][1] - key[1][0], n1, n2, False)
        entry["held"] = held
        result["sweeps"][sweep] = entry
        print(f"sweep {sweep}: " + ", ".join(f"{leg} {entry[leg]['median_ms']:.1f} ms" for leg in LEGS)
              + f"; bit-equal {same}; layer cache {entry['layer_cache']}; held {held}", flush=True)
        if sweep == "shift":
            # the listed copies, timed by the library's profiler: a capture frame (a fresh cache's second frame) and a reuse frame
            copies = {}
            fresh = stnerf_amd.LayerCache()
            model.set_background_cache(None)
            model.set_layer_cache(fresh)
            render(sweep, -1)
            for name, kind in (("capture", 1), ("restore", 0)):
                ops.profile_begin()
                render(sweep, -1)
                recs = [r for r in ops.profile_end() if r["kernel"] == "copy_layer_raw_listed" and r["kind"] == kind]
                nbytes, ms = sum(r["n_rays"] * r["bytes_per_ray"] for r in recs), sum(r["ms"] for r in recs)
                copies[name] = dict(launches=len(recs), GB=nbytes / 1e9, ms=ms, GBps=(nbytes / 1e9) / (ms / 1e3) if ms > 0 else None)
            result["copies"] = copies
            print(f"listed copies: {copies}", flush=True)
            del fresh
        model.set_background_cache(None)
        model.set_layer_cache(None)
        del caches
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        lines = [f"| sweep | {' | '.join(LEGS)} | bit-equal |", "|---|---|---|---|---|"]
        for sweep, e in result["sweeps"].items():
            cell = lambda leg: f"{e[leg]['median_ms']:.1f} ({e[leg]['min_ms']:.1f} .. {e[leg]['max_ms']:.1f})"
            lines.append(f"| {sweep} | {' | '.join(cell(leg) for leg in LEGS)} | {e['bit_equal']} |")
        lines += ["", "| layer | entries | hit rays | bytes held | dense bytes | ratio |", "|---|---|---|---|---|---|"]
        for layer, d in sorted(result["sweeps"]["fade"]["held"].items()):
            lines.append(f"| {layer} | {d['entries']} | {d['hit_rays']} | {d['bytes']} | {d['dense_bytes']} | {d['bytes'] / d['dense_bytes']:.3f} |")
        lines += ["", "| listed copy | launches | GB (read + write) | ms | GB/s |", "|---|---|---|---|---|"]
        for name, c in result.get("copies", {}).items():
            lines.append(f"| {name} | {c['launches']} | {c['GB']:.3f} | {c['ms']:.3f} | {c['GBps'] and round(c['GBps'])} |")
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
