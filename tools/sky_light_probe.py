#!/usr/bin/env python3
"""What light rays aimed at the sky's image cost and buy (RWR_FLAG_LIGHT_SKY), on tools/sky_image_probe.py's two workloads
under its synthetic place (a sun of radiance 50 four degrees across) as an n = 256 map - same camera, spp, bounces and binary:

  time    ms per frame under RWR_FLAG_SKY_IMAGE alone (A) against the same frame with RWR_FLAG_LIGHT_SKY | RWR_FLAG_LIGHT_MIS (B),
          alternated over --repeats rounds, 2 frames in flight, mean and spread (min..max) of each side;
  counts  rwr_last_light_stats and rwr_last_sky_light_stats of a B frame;
  MSE     of one 16-spp frame against 2 048 accumulated plain samples (another seed), over the whole frame: A, B (equal samples) and
          A at round(16 * t_B / t_A) samples (equal time).

One JSON line per workload.  The A side is also the figure to hold against the parent commit's build of the same frame (RWR_HIP_LIB
names the other build's library, --image-only leaves B out for it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402
from sky_image_probe import place  # noqa: E402
from sky_probe import make_ctx, time_frames  # noqa: E402

rwr = graft.load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--image-only", action="store_true")
    args = ap.parse_args()
    with_flag = hasattr(rwr.lib(), "rwr_last_sky_light_stats") and not args.image_only
    sun = rwr.sky_image_from_equirect(place(), 256)
    work = (("1080p suzanne", bench.CONFIGS["cfg3"], 64, 1), ("configs[3] 4K x16", bench.CONFIGS["cfg4"], 16, 2))
    for name, cfg, spp, bounces in work:
        ctx, cam = make_ctx(cfg)
        ctx.sky_set_image(sun)
        base = (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE
        on = base | (rwr.FLAG_LIGHT_SKY | rwr.FLAG_LIGHT_MIS if with_flag else 0)
        plain = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=base))
        lit = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=on)) if with_flag else None
        out = dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=bounces, frames_in_flight=2, frames=args.frames,
                   repeats=args.repeats, library=os.environ.get("RWR_HIP_LIB", "this tree's"), map_side=256)
        times = {"image": [], "light_sky": []}
        for _ in range(args.repeats):
            times["image"].append(time_frames(ctx, plain, args.frames))
            if with_flag:
                times["light_sky"].append(time_frames(ctx, lit, args.frames))
        for k, v in times.items():
            if v:
                out[k + "_ms"] = round(float(np.mean(v)), 4)
                out[k + "_spread"] = [round(min(v), 4), round(max(v), 4)]
        if with_flag:
            ratio = float(np.mean(times["light_sky"])) / float(np.mean(times["image"]))
            out["light_sky_over_image"] = round(ratio, 4)
            lit()
            ctx.synchronize()
            out["bounce_rays"] = int(ctx.last_render_stats()[1])
            out["light_stats"] = list(ctx.last_light_stats())
            out["sky_light_stats"] = list(ctx.last_sky_light_stats())
            # the truth: 2 048 plain samples, accumulated 32 at a time
            ctx.set_frames_in_flight(1)
            ctx.accum_reset()
            aux = rwr.FLAG_AUX_OUTPUTS
            acc = rwr.make_params(spp=32, max_bounces=bounces, seed=77, flags=base | aux | rwr.FLAG_ACCUMULATE)
            for _ in range(64):
                ctx.render(cam, acc)
            truth = ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)
            ctx.accum_reset()

            def mse(flags, n):
                ctx.render(cam, rwr.make_params(spp=n, max_bounces=bounces, seed=5, flags=flags | aux))
                return float(((ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64) - truth) ** 2).mean())

            more = max(16, int(round(16 * ratio)))
            out.update(mse_16spp_image=mse(base, 16), mse_16spp_light_sky=mse(on, 16), equal_time_spp=more, mse_equal_time_image=mse(base, more))
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
