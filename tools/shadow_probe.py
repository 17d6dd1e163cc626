#!/usr/bin/env python3
"""Cost of shadow rays (RWR_FLAG_SHADOWS): ms per frame with the flag against the SAME frame without it, alternated
in one process (block of frames without, block with, --repeats times), 2 frames in flight, on
  1080p suzanne at 1 and 16 spp with 1 bounce, configs[3]'s 4K x16 grid at 16 spp with 1 bounce, the closed room (camera inside
  cube.obj, 1080p, 4 spp) at 4 bounces.
One JSON line per configuration: mean and spread (min..max over the repeats) both ways, the ratio, shadow rays and occluded share.
RWR_HIP_LIB picks the library (a build of the parent commit for the frames without the flag: --no-flag-only times those alone).

--trace I: render --frames frames of configuration I with the flag and nothing else, for a run of its own under
rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def configurations():
    import bench
    room = dict(scene="cube.obj", width=1920, height=1080, camera=dict(eye=(0.1, 0.2, 0.3), target=(0.0, 0.0, -1.0)), no_spheres=True)
    return (("1080p suzanne spp 1 B 1", bench.CONFIGS["cfg3"], 1, 1), ("1080p suzanne spp 16 B 1", bench.CONFIGS["cfg3"], 16, 1),
            ("configs[3] 4K x16 spp 16 B 1", bench.CONFIGS["cfg4"], 16, 1), ("closed room 1080p spp 4 B 4", room, 4, 4))


def params(rwr, spp, b, shadows):
    flags = (rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | (getattr(rwr, "FLAG_SHADOWS", 1 << 7) if shadows else 0)
    return rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=flags)


def make_ctx(rwr, cfg):
    w, h = cfg["width"], cfg["height"]
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute(cfg["scene"]))
    ctx.set_spheres(rwr.make_spheres([]) if cfg.get("no_spheres") else rwr.make_spheres())
    if cfg.get("instances"):
        ctx.set_instances(rwr.make_instance_grid(cfg["instances"], 3.0))
    ctx.resize(w, h)
    ctx.set_frames_in_flight(2)
    cam = rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, **cfg["camera"]))
    return ctx, cam


def time_frames(ctx, call, frames):
    for _ in range(3):
        call()
    ctx.synchronize()
    ctx.timer_begin()
    for _ in range(frames):
        call()
    return ctx.timer_end() / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--trace", type=int, default=None, metavar="I")
    ap.add_argument("--no-flag-only", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    for i, (name, cfg, spp, b) in enumerate(configurations()):
        if args.trace is not None and i != args.trace:
            continue
        ctx, cam = make_ctx(rwr, cfg)
        plain = ctx.render_call(cam, params(rwr, spp, b, False))
        if args.trace is not None:
            call = ctx.render_call(cam, params(rwr, spp, b, True))
            for _ in range(args.frames):
                call()
            ctx.synchronize()
            ctx.close()
            continue
        t_off, t_on = [], []
        shadowed = None if args.no_flag_only else ctx.render_call(cam, params(rwr, spp, b, True))
        for _ in range(args.repeats):
            t_off.append(time_frames(ctx, plain, args.frames))
            if shadowed:
                t_on.append(time_frames(ctx, shadowed, args.frames))
        row = dict(config=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames,
                   repeats=args.repeats, ms_without=round(float(np.mean(t_off)), 4), spread_without=[round(min(t_off), 4), round(max(t_off), 4)])
        if shadowed:
            ctx.render(cam, params(rwr, spp, b, True))
            rays, occluded = ctx.last_shadow_stats()
            row.update(ms_with=round(float(np.mean(t_on)), 4), spread_with=[round(min(t_on), 4), round(max(t_on), 4)],
                       ratio=round(float(np.mean(t_on) / np.mean(t_off)), 3), shadow_rays=rays, occluded_share=round(occluded / max(rays, 1), 4))
        print(json.dumps(row), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
