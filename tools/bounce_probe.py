#!/usr/bin/env python3
"""Cost of deeper paths (RWR_FLAG_MULTI_BOUNCE): ms per frame against max_bounces B = 0, 1, 2, 4, 8 at 16 spp,
2 frames in flight, on 1080p suzanne (bench.py cfg3's camera) and configs[3]'s 4K x16 instanced grid (cfg4).  Every B is timed
--repeats times over --frames frames; one JSON line per (workload, B) with the mean, the spread (min..max) and the bounce rays
of one frame.

--trace B [--workload I]: render --frames frames of workload I (0: 1080p, 1: 4K grid) at that B and nothing else, for a run of its own under
rocprofv3 --kernel-trace --stats; --summarize DIR B: the time per generation from such a run's kernel statistics (the sort and
trace kernels of all generations / (frames x launch groups x B))."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

BOUNCES = (0, 1, 2, 4, 8)
SPP = 16


def workloads():
    import bench
    return (("1080p suzanne", bench.CONFIGS["cfg3"]), ("configs[3] 4K x16", bench.CONFIGS["cfg4"]))


def params(rwr, b):
    return rwr.make_params(spp=SPP, max_bounces=b, seed=3, flags=rwr.FLAG_MULTI_BOUNCE if b > 1 else 0)


def make_ctx(rwr, cfg):
    w, h = cfg["width"], cfg["height"]
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute(cfg["scene"]))
    ctx.set_spheres(rwr.make_spheres())
    if cfg.get("instances"):
        ctx.set_instances(rwr.make_instance_grid(cfg["instances"], 3.0))
    ctx.resize(w, h)
    ctx.set_frames_in_flight(2)
    cam = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, **cfg["camera"]))
    return ctx, cam


def time_frames(ctx, call, frames):
    import torch
    for _ in range(4):
        call()
    torch.cuda.synchronize()
    ctx.timer_begin()
    for _ in range(frames):
        call()
    return ctx.timer_end() / frames


def kernel_rows(d):
    """(kernel name, calls, total ns) from a rocprofv3 run under d: its kernel_stats CSV, or its results database."""
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            yield (row.get("Name") or row.get("KernelName") or "", int(float(row.get("Calls") or 0)),
                   float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0))
    for f in glob.glob(os.path.join(d, "**", "*results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(f) as db:
            yield from db.execute("select name, count(*), sum(duration) from kernels group by name")


def summarize(d, b, frames):
    """Per-generation time from a rocprofv3 --kernel-trace --stats run under d."""
    tot, calls = {}, {}
    for name, n, ns in kernel_rows(d):
        for k in ("k_wf_sort", "k_wf_trace_packet", "k_wf_trace_lane", "k_wf_primary", "k_wf_resolve"):
            if k in name:
                tot[k] = tot.get(k, 0.0) + ns
                calls[k] = calls.get(k, 0) + n
    if not tot:
        raise SystemExit(f"no kernel statistics under {d}")
    bounce_ns = tot.get("k_wf_sort", 0.0) + tot.get("k_wf_trace_packet", 0.0) + tot.get("k_wf_trace_lane", 0.0)
    sorts = calls.get("k_wf_sort", 0)   # one per launch group and generation
    return dict(bounces=b, kernels_ms={k: round(v * 1e-6, 3) for k, v in sorted(tot.items())}, calls=calls,
                generations=sorts, us_per_generation=round(bounce_ns * 1e-3 / sorts, 1) if sorts else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--trace", type=int, default=None, metavar="B")
    ap.add_argument("--workload", type=int, default=None, help="--trace: this workload only (0 or 1)")
    ap.add_argument("--summarize", nargs=2, metavar=("DIR", "B"))
    args = ap.parse_args()
    if args.summarize:
        print(json.dumps(summarize(args.summarize[0], int(args.summarize[1]), args.frames)), flush=True)
        return
    import __graft_entry__ as graft
    rwr = graft.load_package()
    for i, (name, cfg) in enumerate(workloads()):
        if args.workload is not None and i != args.workload:
            continue
        ctx, cam = make_ctx(rwr, cfg)
        if args.trace is not None:
            call = ctx.render_call(cam, params(rwr, args.trace))
            for _ in range(args.frames):
                call()
            ctx.synchronize()
            ctx.close()
            continue
        for b in BOUNCES:
            call = ctx.render_call(cam, params(rwr, b))
            t = [time_frames(ctx, call, args.frames) for _ in range(args.repeats)]
            ctx.render(cam, params(rwr, b))
            rays = ctx.last_render_stats()
            print(json.dumps(dict(workload=name, width=cfg["width"], height=cfg["height"], spp=SPP, bounces=b, frames_in_flight=2,
                                  frames=args.frames, repeats=args.repeats, ms=round(float(np.mean(t)), 4),
                                  spread=[round(min(t), 4), round(max(t), 4)], primary_rays=rays[0], bounce_rays=rays[1])), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
