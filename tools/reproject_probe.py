#!/usr/bin/env python3
"""Cost of temporal reprojection (RWR_FLAG_REPROJECT): ms per frame of a frame without the flag (A, rendered with
RWR_FLAG_AUX_OUTPUTS: the planes the stage implies) against one with it (B), same spp and bounce, alternated A/B over --repeats
rounds of --frames frames, 2 frames in flight, one process.  The camera takes one controller step per frame on both sides (ten
to the right, ten back, small steps), so B's taps land between pixels as they do in use.  Workloads: 1080p suzanne (bench.py
cfg3's camera) at 1 and 16 spp + bounce, configs[3]'s 4K x16 instanced grid (cfg4) at 1 spp + bounce.  Prints one JSON line per
workload with the mean and the spread (min..max) of each side and the share of the hit pixels B's last frame reused.

--plain-only: side A alone - for a library of the parent commit named by RWR_HIP_LIB, which lacks the flag (builds alternated
by the caller).  --trace: a few reprojected frames of each workload and nothing else, for a run of its own under
rocprofv3 --kernel-trace --stats (k_wf_reproject per launch against about 24 B read, four taps of 36 B and 56 B written per pixel)."""
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
STEP = 0.02   # controller speed per frame: about 1.1 degrees about the target


def make_ctx(cfg):
    w, h = cfg["width"], cfg["height"]
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute(cfg["scene"]))
    ctx.set_spheres(rwr.make_spheres())
    if cfg.get("instances"):
        ctx.set_instances(rwr.make_instance_grid(cfg["instances"], 3.0))
    ctx.resize(w, h)
    ctx.set_frames_in_flight(2)
    return ctx, rwr.make_camera(aspect=w / h, **cfg["camera"])


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
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    work = (("1080p suzanne", bench.CONFIGS["cfg3"], 1), ("1080p suzanne", bench.CONFIGS["cfg3"], 16), ("configs[3] 4K x16", bench.CONFIGS["cfg4"], 1))
    keys = [rwr.KEY_RIGHT] * 10 + [rwr.KEY_LEFT] * 10
    for name, cfg, spp in work:
        ctx, cam = make_ctx(cfg)
        plain = rwr.make_params(spp=spp, max_bounces=1, seed=3, flags=rwr.FLAG_AUX_OUTPUTS)
        call_a = ctx.loop_call(cam.copy(), keys, plain, speed=STEP)
        out = dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=1, frames_in_flight=2, frames=args.frames,
                   repeats=args.repeats, library=os.path.relpath(rwr.LIB_PATH, ROOT))
        if args.plain_only:
            a = [time_frames(ctx, call_a, args.frames) for _ in range(args.repeats)]
            out.update(plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)])
            print(json.dumps(out), flush=True)
            ctx.close()
            continue
        rp = rwr.make_params(spp=spp, max_bounces=1, seed=3, flags=rwr.FLAG_REPROJECT)
        call_b = ctx.loop_call(cam.copy(), keys, rp, speed=STEP)
        if args.trace:
            for _ in range(args.frames):
                call_b()
            ctx.synchronize()
            ctx.close()
            continue
        a, b = [], []
        for _ in range(args.repeats):
            a.append(time_frames(ctx, call_a, args.frames))
            b.append(time_frames(ctx, call_b, args.frames))
        reused, fresh, background = ctx.last_reproject_stats()
        pixels = cfg["width"] * cfg["height"]
        out.update(params=ctx.reproject_params(), history_frames=ctx.reproject_frames(), reused_share_of_hits=round(reused / max(1, reused + fresh), 4),
                   background_share=round(background / pixels, 4),
                   plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)],
                   reproject_ms=round(float(np.mean(b)), 4), reproject_spread=[round(min(b), 4), round(max(b), 4)],
                   reproject_minus_plain_us=round((float(np.mean(b)) - float(np.mean(a))) * 1e3, 1),
                   planned_bytes_per_frame=(24 + 4 * 36 + 56) * pixels)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
