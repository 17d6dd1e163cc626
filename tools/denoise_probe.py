#!/usr/bin/env python3
"""Cost of the a-trous denoiser (RWR_FLAG_DENOISE): ms per frame of a frame without the flag (A, rendered with
RWR_FLAG_AUX_OUTPUTS: the planes the filter implies) against one with it (B), same camera, spp and bounce, alternated A/B over
--repeats rounds, 2 frames in flight.  Workloads: 1080p suzanne (bench.py cfg3's camera) at 1 and 16 spp + bounce, configs[3]'s
4K x16 instanced grid (cfg4) at 1 spp + bounce.  Prints one JSON line per workload with the mean and the spread (min..max) of
each side; the filter's parameters are the context's defaults unless --iterations / --sigma say otherwise.

--trace: render a few denoised frames of each workload and nothing else - for a run of its own under
rocprofv3 --kernel-trace --stats (k_dn_guide, k_dn_tile<1|2>, k_dn_far per launch against 25 taps x 32 B per pixel from cache)."""
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
    ap.add_argument("--iterations", type=int)
    ap.add_argument("--sigma", type=float)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    work = (("1080p suzanne", bench.CONFIGS["cfg3"], 1), ("1080p suzanne", bench.CONFIGS["cfg3"], 16), ("configs[3] 4K x16", bench.CONFIGS["cfg4"], 1))
    for name, cfg, spp in work:
        ctx, cam = make_ctx(cfg)
        ctx.set_denoise_params(iterations=args.iterations, sigma_color=args.sigma)
        plain = rwr.make_params(spp=spp, max_bounces=1, seed=3, flags=rwr.FLAG_AUX_OUTPUTS)
        dn = rwr.make_params(spp=spp, max_bounces=1, seed=3, flags=rwr.FLAG_DENOISE)
        call_a, call_b = ctx.render_call(cam, plain), ctx.render_call(cam, dn)
        if args.trace:
            for _ in range(args.frames):
                call_b()
            ctx.synchronize()
            ctx.close()
            continue
        call_a()
        before = ctx.readback(aux=True)
        call_b()
        after = ctx.readback(aux=True)
        guides_equal = all(before[k].tobytes() == after[k].tobytes() for k in ("depth", "obj_id", "hit_t"))
        moved = float(np.abs(after["color_f32"] - before["color_f32"]).max())
        a, b = [], []
        for _ in range(args.repeats):
            a.append(time_frames(ctx, call_a, args.frames))
            b.append(time_frames(ctx, call_b, args.frames))
        pixels = cfg["width"] * cfg["height"]
        p = ctx.denoise_params()
        print(json.dumps(dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=1, frames_in_flight=2,
                              frames=args.frames, repeats=args.repeats, params=p, guide_planes_unchanged=guides_equal,
                              largest_colour_change=round(moved, 5),
                              plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)],
                              denoise_ms=round(float(np.mean(b)), 4), denoise_spread=[round(min(b), 4), round(max(b), 4)],
                              denoise_minus_plain_us=round((float(np.mean(b)) - float(np.mean(a))) * 1e3, 1),
                              tap_bytes_per_frame=25 * 32 * pixels * p["iterations"])), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
