#!/usr/bin/env python3
"""What layer instances cost (GPU box): the bench's headline shape (taekwondo-1080p-64+64, split bf16, one GPU, whole view per
frame) rendered plain, with K = 1 and K = 3 instances of performer 1, and on the WIDE models with the same layers (DESIGN.md
section 7: LAYER_NUM = L + K, the source's networks copied) -- which compute the same frames bit for bit and should cost the
same time.  The legs ALTERNATE in one process: one warm-up frame per leg, then `--runs` rounds of one frame per leg (frame i of
every leg from pose i), each timed by a host clock around a render that ends in a device synchronise, the launch profiler off.
Also reports the device memory of the packed networks (the distinct blobs the launch would name): the instanced model's is the
plain model's, the wide model's grows with K.

    python tools/bench_instances.py --json instances.json --markdown profiles/instances_ab.md
    python tools/bench_instances.py --record instances.json --markdown profiles/instances_ab.md      # the table from a saved record (no GPU)
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--json", default=None, help="write the record here too")
ap.add_argument("--markdown", default=None, help="write the table here")
ap.add_argument("--record", default=None, help="a saved record: measure nothing, only write the table")
ap.add_argument("--note", default=None, help="a closing line for the table's file")
args = ap.parse_args()
WORKLOAD = "taekwondo-1080p-64+64"
COMMAND = "python tools/bench_instances.py --json instances.json --markdown profiles/instances_ab.md"


def write_markdown(rec, path):
    lines = ["# Layer instances: A/B on the headline shape", "",
             f"`{COMMAND}`: {WORKLOAD}, split bf16, one MI355X, whole view per frame, L = {rec['L']} performers.  Instances are copies of "
             f"performer 1, shifted apart and shown at their own frame ids; the wide legs are the ordinary models with LAYER_NUM = L + K and "
             f"the source's networks copied (DESIGN.md section 7), which render the same bits.  {rec['warmup']} warm-up frame(s) per leg, then "
             f"{rec['runs']} rounds of one frame per leg, the legs alternating inside a round (frame i of every leg from pose i); host clock "
             "around a render that ends in a device synchronise, launch profiler off.", "",
             "| leg | layers l | frame ms (round 1, 2, 3) | mean | spread | packed networks, MiB | hit rays per layer (last frame) |", "|---|---|---|---|---|---|---|"]
    for name, d in rec["legs"].items():
        ms = d["frame_ms"]
        lines.append(f"| {name} | {d['l']} | {', '.join(f'{x:.1f}' for x in ms)} | {sum(ms) / len(ms):.1f} | {max(ms) - min(ms):.1f} | "
                     f"{d['packed_bytes'] / 2**20:.2f} | {', '.join(str(x) for x in d['hits'])} |")
    legs = rec["legs"]
    mean = lambda k: sum(legs[k]["frame_ms"]) / len(legs[k]["frame_ms"])
    lines.append("")
    for K in rec["Ks"]:
        a, b = f"instanced, K = {K}", f"wide, K = {K}"
        lines.append(f"K = {K}: instanced {mean(a):.1f} ms against wide {mean(b):.1f} ms ({100 * (mean(a) - mean(b)) / mean(b):+.2f} %); against the plain "
                     f"frame {mean(a) - mean('plain'):+.1f} ms ({100 * (mean(a) - mean('plain')) / mean('plain'):+.1f} %): the sampler, the stage kernel, the "
                     f"compositor and the resampler on {legs[a]['l']} layers instead of {legs['plain']['l']}.  Packed networks: instanced "
                     f"{legs[a]['packed_bytes'] / 2**20:.2f} MiB = plain {legs['plain']['packed_bytes'] / 2**20:.2f} MiB, wide {legs[b]['packed_bytes'] / 2**20:.2f} MiB "
                     f"(+{(legs[b]['packed_bytes'] - legs['plain']['packed_bytes']) / 2**20:.2f}).  Outputs of the two legs bit-identical on the last "
                     f"frame: {legs[a]['equals_wide']}.")
    if args.note or rec.get("note"):
        lines += ["", args.note or rec["note"]]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if args.record:
    write_markdown(json.load(open(args.record)), args.markdown)
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from stnerf_amd import synthetic as syn  # noqa: E402
from stnerf_amd.modeling import build_layered_model  # noqa: E402
from stnerf_amd.parallel import render_view  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_instances.py measures on the GPU: none here (nothing is measured on the CPU)")

Ks = (1, 3)
SRC = 1


def scene():
    model, shape = bench.build_scene(WORKLOAD, "cuda")
    model.set_precision("bf16x3")
    return model, shape


def edits(L, K):
    """Per-layer shift list: the instances stand apart from their source (None without instances: the plain frame)."""
    if K == 0:
        return None
    return [[0.0, 0.0, 0.0] for _ in range(L + 1)] + [[0.45 * (k + 1), 0.0, -0.35 * (k + 1)] for k in range(K)]


def wide_of(model, shape):
    """W(M): LAYER_NUM = L + K, the source's modules and box column copied, every other setting the same."""
    H, W, L, n1, n2, st, dt = shape
    K = len(model.instances)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for j, src in enumerate(model.instances):
        for lst in ("spacenets", "spacenets_fine", "time_deform_nets"):
            head = f"{lst}.{src - 1}."
            for k in [k for k in sd if k.startswith(head)]:
                sd[f"{lst}.{L + j}." + k[len(head):]] = sd[k].clone()
    wide = build_layered_model(bench.make_cfg(L + K, n1, n2, st, dt), camera_num=1)
    wide.load_state_dict(sd)
    wide = wide.cuda().eval()
    wide.set_precision("bf16x3")
    bb = model.bboxes
    wide.set_bkgd_bbox(model.bkgd_bbox)
    wide.set_bboxes(torch.cat([bb] + [bb[:, s - 1:s].clone() for s in model.instances], 1))
    wide.shift = model.shift
    return wide


def packed_bytes(model):
    """Device bytes of the distinct packed blobs a launch of this model names."""
    prec = model.bkgd_spacenet.precision
    mods = [model.bkgd_spacenet, model.bkgd_spacenet_fine]
    for i in range(1, model.total_layers):
        j = model._module_index(i)
        mods += [model.spacenets[j], model.spacenets_fine[j]] + ([model.time_deform_nets[j]] if model.use_deform_time else [])
    blobs = {m._packed(prec).blob.data_ptr(): m._packed(prec).blob for m in mods}
    return sum(b.numel() * b.element_size() for b in blobs.values())


models = {}
plain, shape = scene()
H, W, L = shape[0], shape[1], shape[2]
models["plain"] = plain
for K in Ks:
    m, _ = scene()
    for _ in range(K):
        m.add_instance(SRC)
    m.shift = edits(L, K)
    models[f"instanced, K = {K}"] = m
    models[f"wide, K = {K}"] = wide_of(m, shape)


def frame_ids(model):
    K = model.total_layers - 1 - L
    return [1.0] + [2.5] * L + [1.5, 2.0, 3.0, 1.0][:K]


def frame(model, i):
    Kc, T = syn.camera(H, W, orbit_deg=10.0 + 1.5 * i)
    model.seed = i
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        out = render_view(model, Kc, T, H, W, frame_ids(model))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


times = {name: [] for name in models}
last = {}
for i in range(args.warmup):
    for name, m in models.items():
        frame(m, -1 - i)
for i in range(args.runs):
    for name, m in models.items():
        ms, out = frame(m, i)
        times[name].append(round(ms, 2))
        last[name] = out if i == args.runs - 1 else None

flat = lambda out: [t for trip in (out[0], out[1]) for t in trip] + [t for k in (2, 3) for trip in out[k] for t in trip] + list(out[4])
legs = {}
for name, m in models.items():
    d = dict(l=m.total_layers, frame_ms=times[name], packed_bytes=packed_bytes(m), hits=[int(x.sum()) for x in last[name][4]])
    if name.startswith("instanced"):
        other = last[name.replace("instanced", "wide")]
        d["equals_wide"] = all(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)) for a, b in zip(flat(last[name]), flat(other)))
    legs[name] = d
rec = dict(workload=WORKLOAD, precision="bf16x3", L=L, Ks=list(Ks), runs=args.runs, warmup=args.warmup, legs=legs, note=args.note)
print(json.dumps(rec))
if args.json:
    with open(args.json, "w") as f:
        json.dump(rec, f)
if args.markdown:
    write_markdown(rec, args.markdown)
