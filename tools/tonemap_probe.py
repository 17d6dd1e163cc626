#!/usr/bin/env python3
"""Cost of the tone-mapping stage (RWR_FLAG_TONEMAP): ms per frame of a frame without the flag (rendered with
RWR_FLAG_AUX_OUTPUTS: the planes the stage implies) against one with it in manual mode (one launch: k_tm_apply) and one with
auto-exposure (a memset and three launches: k_tm_measure, k_tm_exposure, k_tm_apply), same camera, spp and bounce, alternated over
--repeats rounds, 2 frames in flight.  Workloads: 1080p suzanne at 64 spp + bounce (bench.py cfg3), the 4K x16 instanced grid at
16 spp + bounce (cfg4).  Prints one JSON line per workload with the median (times[len // 2], as bench.py takes it) and the spread
(min..max) of each side, and the bytes the stage moves by its definition: 20 B per pixel in manual mode, 36 B with the measure."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ctx.timer_begin()
    for _ in range(frames):
        call()
    return ctx.timer_end() / frames


def median(times):
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10)
    args = ap.parse_args()
    for name, cfg in (("1080p suzanne", bench.CONFIGS["cfg3"]), ("configs[3] 4K x16", bench.CONFIGS["cfg4"])):
        ctx, cam = make_ctx(cfg)
        spp, bounces = cfg["spp"], cfg["bounces"]
        plain = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=rwr.FLAG_AUX_OUTPUTS))
        mapped = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=rwr.FLAG_TONEMAP))
        sides = {"plain": [], "manual": [], "auto": []}
        stats = None
        for _ in range(args.repeats):
            sides["plain"].append(time_frames(ctx, plain, args.frames))
            ctx.set_tonemap_params(curve=rwr.TONEMAP_ACES, auto_exposure=0)
            sides["manual"].append(time_frames(ctx, mapped, args.frames))
            ctx.set_tonemap_params(curve=rwr.TONEMAP_ACES, auto_exposure=1)
            sides["auto"].append(time_frames(ctx, mapped, args.frames))
            stats = ctx.last_tonemap_stats()
        pixels = cfg["width"] * cfg["height"]
        out = dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=bounces, frames_in_flight=2, frames=args.frames,
                   repeats=args.repeats, counted_pixels=stats[1], exposure=round(stats[2], 6), manual_bytes=20 * pixels, auto_bytes=36 * pixels)
        for k, t in sides.items():
            out[k + "_ms"] = round(median(t), 4)
            out[k + "_spread"] = [round(min(t), 4), round(max(t), 4)]
        for k in ("manual", "auto"):
            out[k + "_minus_plain_us"] = round((median(sides[k]) - median(sides["plain"])) * 1e3, 1)
            out[k + "_share_of_frame"] = round((median(sides[k]) - median(sides["plain"])) / median(sides["plain"]), 5)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
