#!/usr/bin/env python3
"""Cost of the sky light (RWR_FLAG_SKY): ms per frame of a frame without the flag (A) against the same frame with it
(B) - same camera, spp, bounces and binary - alternated A/B over --repeats rounds, 2 frames in flight.  Workloads: 1080p suzanne
(bench.py cfg3's camera) at 1 and 16 spp + 1 bounce, and configs[3]'s 4K x16 instanced grid (cfg4) at 16 spp + 2 bounces.
Prints one JSON line per workload with the mean and the spread (min..max) of each side, and checks on the way that the sky
changes the frame and leaves the ray counts alone.  The plain side is the figure to hold against the parent commit's for the
same frame: the flag must cost nothing where it is off."""
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
    args = ap.parse_args()
    work = (("1080p suzanne", bench.CONFIGS["cfg3"], 1, 1), ("1080p suzanne", bench.CONFIGS["cfg3"], 16, 1),
            ("configs[3] 4K x16", bench.CONFIGS["cfg4"], 16, 2))
    for name, cfg, spp, bounces in work:
        ctx, cam = make_ctx(cfg)
        deep = rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0
        plain = rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep)
        sky = rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep | rwr.FLAG_SKY)
        call_a, call_b = ctx.render_call(cam, plain), ctx.render_call(cam, sky)
        # on the way: the sky lights the frame, with the same rays
        call_a()
        off, rays_off = ctx.readback()["color"], ctx.last_render_stats()
        call_b()
        on, rays_on = ctx.readback()["color"], ctx.last_render_stats()
        a, b = [], []
        for _ in range(args.repeats):
            a.append(time_frames(ctx, call_a, args.frames))
            b.append(time_frames(ctx, call_b, args.frames))
        print(json.dumps(dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=bounces, frames_in_flight=2,
                              frames=args.frames, repeats=args.repeats, frame_changed=bool((on != off).any()),
                              never_darker=bool((on >= off).all()), same_rays=bool(rays_on == rays_off), bounce_rays=int(rays_on[1]),
                              plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)],
                              sky_ms=round(float(np.mean(b)), 4), sky_spread=[round(min(b), 4), round(max(b), 4)],
                              sky_minus_plain_us=round((float(np.mean(b)) - float(np.mean(a))) * 1e3, 1))), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
