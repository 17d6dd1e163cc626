#!/usr/bin/env python3
"""Cost of soft shadows (RWR_FLAG_SOFT_SHADOWS, DESIGN §6 Cost): ms per frame of the hard-shadow frame (RWR_FLAG_SHADOWS) against the
SAME frame with lights of radius 0.05 and of radius 0.2, alternated in one process (a block of hard frames, a block of each soft
arm, --repeats times), 2 frames in flight, tools/shadow_probe.py's protocol, on its two large cases:
  1080p suzanne at 16 spp with 1 bounce, configs[3]'s 4K x16 grid at 16 spp with 1 bounce.
One JSON line per case: mean and spread (min..max over the repeats) of every arm, the ratios, shadow rays and occluded shares.

--hard-only times the hard frame alone and touches no entry point of the feature: what a library without it (RWR_HIP_LIB, a build
of the parent commit) can run - the figure to hold against this build's hard arm: the flag must cost nothing where it is off.
Alternate the two libraries' runs in one session.

--trace I [--radius R]: render --frames frames of case I with the flag and nothing else, for a run of its own under
rocprofv3 --kernel-trace --stats (R = 0: the hard frame)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def cases():
    import bench
    return (("1080p suzanne spp 16 B 1", bench.CONFIGS["cfg3"], 16, 1), ("configs[3] 4K x16 spp 16 B 1", bench.CONFIGS["cfg4"], 16, 1))


def params(rwr, spp, b, soft):
    flags = (rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_SHADOWS | (rwr.FLAG_SOFT_SHADOWS if soft else 0)
    return rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=flags)


def make_ctx(rwr, cfg):
    w, h = cfg["width"], cfg["height"]
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute(cfg["scene"]))
    ctx.set_spheres(rwr.make_spheres())
    if cfg.get("instances"):
        ctx.set_instances(rwr.make_instance_grid(cfg["instances"], 3.0))
    ctx.resize(w, h)
    ctx.set_frames_in_flight(2)
    return ctx, rwr.camera_build_inv_uniform(rwr.make_camera(aspect=w / h, **cfg["camera"]))


def time_frames(ctx, call, frames):
    import torch
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ctx.timer_begin()
    for _ in range(frames):
        call()
    return ctx.timer_end() / frames


def stats(v):
    return dict(ms=round(float(np.mean(v)), 4), spread=[round(min(v), 4), round(max(v), 4)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--hard-only", action="store_true")
    ap.add_argument("--trace", type=int, default=-1)
    ap.add_argument("--radius", type=float, default=0.2)
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    work = cases()
    if args.trace >= 0:
        name, cfg, spp, b = work[args.trace]
        ctx, cam = make_ctx(rwr, cfg)
        if args.radius > 0.0:
            ctx.shadow_set_params(args.radius, args.radius)
        call = ctx.render_call(cam, params(rwr, spp, b, args.radius > 0.0))
        for _ in range(args.frames):
            call()
        ctx.readback()
        print(json.dumps(dict(case=name, radius=args.radius, frames=args.frames, shadow_stats=ctx.last_shadow_stats())), flush=True)
        ctx.close()
        return
    for name, cfg, spp, b in work:
        ctx, cam = make_ctx(rwr, cfg)
        hard = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=(rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_SHADOWS))
        hard()
        ctx.readback()
        rays_hard = ctx.last_shadow_stats()
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats,
                   library=os.environ.get("RWR_HIP_LIB") or "this build", shadow_rays=int(rays_hard[0]), occluded_hard=int(rays_hard[1]))
        if args.hard_only:
            out["hard"] = stats([time_frames(ctx, hard, args.frames) for _ in range(args.repeats)])
        else:
            soft = ctx.render_call(cam, params(rwr, spp, b, True))
            arms = {"hard": [], "soft_0.05": [], "soft_0.2": []}
            for r in (0.05, 0.2):   # on the way: the same number of shadow rays, another frame
                ctx.shadow_set_params(r, r)
                soft()
                ctx.readback()
                n, occ = ctx.last_shadow_stats()
                assert n == rays_hard[0], (n, rays_hard)
                out[f"occluded_soft_{r}"] = int(occ)
            for _ in range(args.repeats):
                arms["hard"].append(time_frames(ctx, hard, args.frames))
                for r in (0.05, 0.2):
                    ctx.shadow_set_params(r, r)
                    arms[f"soft_{r}"].append(time_frames(ctx, soft, args.frames))
            for k, v in arms.items():
                out[k] = stats(v)
            for r in (0.05, 0.2):
                out[f"soft_{r}_over_hard"] = round(float(np.mean(arms[f"soft_{r}"]) / np.mean(arms["hard"])), 4)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
