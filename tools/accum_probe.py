#!/usr/bin/env python3
"""Cost of progressive accumulation (RWR_FLAG_ACCUMULATE): ms per frame of a frame without the flag (A) against an
accumulating one (B) with the same camera, spp and bounce, alternated A/B over --repeats rounds, 2 frames in flight.  Workloads:
1080p suzanne (bench.py cfg3's camera) and configs[3]'s 4K x16 instanced grid (cfg4), each at 1 spp + bounce and 16 spp + bounce.
Prints one JSON line per (workload, spp) with the mean and the spread (min..max) of each side, and checks on the way that an
accumulation of K frames is the bytes of one frame of K * spp.

--trace: render a few accumulating frames of each workload and nothing else — for a run of its own under
rocprofv3 --kernel-trace --stats (k_wf_resolve_accum's time against its 64 B per pixel of history traffic)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402

rwr = graft.load_package()


def make_ctx(cfg):
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
    for _ in range(4):
        call()
    torch.cuda.synchronize()
    ctx.timer_begin()
    for _ in range(frames):
        call()
    return ctx.timer_end() / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    work = (("1080p suzanne", bench.CONFIGS["cfg3"]), ("configs[3] 4K x16", bench.CONFIGS["cfg4"]))
    for name, cfg in work:
        ctx, cam = make_ctx(cfg)
        for spp in (1, 16):
            plain = rwr.make_params(spp=spp, max_bounces=1, seed=3)
            acc = rwr.make_params(spp=spp, max_bounces=1, seed=3, flags=rwr.FLAG_ACCUMULATE)
            call_a, call_b = ctx.render_call(cam, plain), ctx.render_call(cam, acc)
            if args.trace:
                for _ in range(args.frames):
                    call_b()
                ctx.synchronize()
                continue
            # the contract on the way: 3 accumulated frames == one frame of 3 spp (or more)
            ctx.accum_reset()
            for _ in range(3):
                call_b()
            got = ctx.readback()
            n = ctx.accum_samples()
            ctx.render(cam, rwr.make_params(spp=n, max_bounces=1, seed=3))
            same = bool(np.array_equal(got["color"], ctx.readback()["color"]))
            a, b = [], []
            for _ in range(args.repeats):
                a.append(time_frames(ctx, call_a, args.frames))
                ctx.accum_reset()
                b.append(time_frames(ctx, call_b, args.frames))
            print(json.dumps(dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=1, frames_in_flight=2,
                                  frames=args.frames, repeats=args.repeats, bytes_equal_to_one_frame=same,
                                  plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)],
                                  accum_ms=round(float(np.mean(b)), 4), accum_spread=[round(min(b), 4), round(max(b), 4)],
                                  accum_minus_plain_us=round((float(np.mean(b)) - float(np.mean(a))) * 1e3, 1),
                                  history_bytes_per_frame=64 * cfg["width"] * cfg["height"])), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
