#!/usr/bin/env python3
"""Cost of the sky's image (RWR_FLAG_SKY_IMAGE): ms per frame of a frame under RWR_FLAG_SKY's gradient (A) against the
same frame under an octahedral map of 256 and of 2048 texels a side (B, C) - same camera, spp, bounces and binary - alternated over
--repeats rounds, 2 frames in flight.  Workloads: 1080p suzanne (bench.py cfg3's camera) at 64 spp + 1 bounce, and configs[3]'s
4K x16 instanced grid (cfg4) at 16 spp + 2 bounces.  One JSON line per workload with the mean and the spread (min..max) of each side.

The gradient side is the figure to hold against the parent commit's for the same frame (it runs the forms the parent has): run this
script once per build, the builds alternated - RWR_HIP_LIB names the other build's library; a library without rwr_sky_set_image
gets the gradient side alone (--gradient-only does the same for this one)."""
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
from sky_probe import make_ctx, time_frames  # noqa: E402

rwr = graft.load_package()


def place(w=1024, h=512):
    """A synthetic latitude-longitude picture of a place: a sky that brightens towards the horizon, a sun of radiance 50 four
    degrees across, a dark ground with a brighter stripe."""
    theta = (np.arange(h) + 0.5) / h * np.pi
    phi = ((np.arange(w) + 0.5) / w - 0.5) * 2.0 * np.pi
    t, p = np.meshgrid(theta, phi, indexing="ij")
    d = np.stack([np.sin(t) * np.sin(p), np.cos(t), -np.sin(t) * np.cos(p)], axis=-1)
    up = np.clip(d[..., 1], 0.0, 1.0)[..., None]
    sky = np.array([0.35, 0.55, 1.0]) * up + np.array([1.0, 0.95, 0.85]) * (1.0 - up)
    ground = np.array([0.12, 0.1, 0.08]) * (1.0 + 2.0 * (np.abs(np.sin(6.0 * p)) > 0.9))[..., None]
    pic = np.where(d[..., 1:2] >= 0.0, sky, ground)
    sun = np.array([0.5, 0.7, -0.5]) / np.linalg.norm([0.5, 0.7, -0.5])
    pic = np.where((d @ sun)[..., None] > np.cos(np.radians(2.0)), 50.0, pic)
    return pic.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--gradient-only", action="store_true")
    args = ap.parse_args()
    with_image = hasattr(rwr.lib(), "rwr_sky_set_image") and not args.gradient_only
    maps = {n: rwr.sky_image_from_equirect(place(), n) for n in (256, 2048)} if with_image else {}
    work = (("1080p suzanne", bench.CONFIGS["cfg3"], 64, 1), ("configs[3] 4K x16", bench.CONFIGS["cfg4"], 16, 2))
    for name, cfg, spp, bounces in work:
        ctx, cam = make_ctx(cfg)
        deep = rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0
        grad = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep | rwr.FLAG_SKY))
        grad()
        base, rays = ctx.readback()["color"], ctx.last_render_stats()
        out = dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=bounces, frames_in_flight=2, frames=args.frames,
                   repeats=args.repeats, library=os.environ.get("RWR_HIP_LIB", "this tree's"), bounce_rays=int(rays[1]))
        times = {"gradient": []}
        image = None
        if with_image:
            image = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep | rwr.FLAG_SKY | rwr.FLAG_SKY_IMAGE))
            for n, m in maps.items():
                ctx.sky_set_image(m)
                image()
                lit, rays_lit = ctx.readback()["color"], ctx.last_render_stats()
                out[f"image_{n}_changes_the_frame"] = bool((lit != base).any())
                out[f"image_{n}_same_rays"] = bool(rays_lit == rays)
                times[f"image_{n}"] = []
        for _ in range(args.repeats):
            times["gradient"].append(time_frames(ctx, grad, args.frames))
            for n, m in maps.items():
                ctx.sky_set_image(m)
                times[f"image_{n}"].append(time_frames(ctx, image, args.frames))
        for k, v in times.items():
            out[k + "_ms"] = round(float(np.mean(v)), 4)
            out[k + "_spread"] = [round(min(v), 4), round(max(v), 4)]
        for n in maps:
            out[f"image_{n}_over_gradient"] = round(float(np.mean(times[f"image_{n}"])) / float(np.mean(times["gradient"])), 4)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
