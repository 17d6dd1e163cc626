#!/usr/bin/env python3
"""Cost of glossy surfaces (RWR_FLAG_GLOSSY): ms per frame of a frame without the flag (A) against the same frame with
it (B) - same camera, spp, bounces, scene, gloss attributes and binary - alternated A/B over --repeats rounds, 2 frames in flight,
tools/mirror_probe.py's protocol.  Workloads, all with 4 bounces and roughness 0.25: the 1080p frame from the reference camera
(bench.py cfg3's, inside the mesh: one or two rays in a frame reach a sphere - what the glossy forms cost when next to nothing glossy is hit) with both of
the reference's spheres glossy at 1 and 16 spp, the same seen from the side (both spheres in view), and configs[3]'s 4K x16
instanced grid (cfg4) with part 0 - the mesh - glossy at 16 spp.  Prints one JSON line per workload with the mean and the spread
(min..max) of each side, the bounce rays of each side, the glossy rays, and the share of the rays that went through pools the sort
classed for the packet kernel (a pass of its own with RWR_WF_STATS=1, outside the timed frames).
--plain-only times side A alone and sets no gloss: what a library without the feature (RWR_HIP_LIB) can run - the figure to hold
against this one's, the flag must cost nothing where it is off."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as graft  # noqa: E402
import bench  # noqa: E402

rwr = graft.load_package()
_POOLS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays")


def make_ctx(cfg, surfaces):
    w, h = cfg["width"], cfg["height"]
    ctx = rwr.Context(0)
    ctx.upload_model(rwr.load_model_compute(cfg["scene"]))
    ctx.set_spheres(rwr.make_spheres())
    if cfg.get("instances"):
        ctx.set_instances(rwr.make_instance_grid(cfg["instances"], 3.0))
    ctx.resize(w, h)
    ctx.set_frames_in_flight(2)
    for kind, index in surfaces:
        (ctx.set_sphere_gloss if kind == "sphere" else ctx.set_part_gloss)(index, 0.25, (1.0, 1.0, 1.0))
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


def packet_share(cfg, surfaces, params):
    """One frame in a context of its own with RWR_WF_STATS=1: (rays in packet-class pools, rays in per-lane-class pools), read from
    what the context prints when it is destroyed."""
    saved = os.environ.get("RWR_WF_STATS")
    os.environ["RWR_WF_STATS"] = "1"
    sys.stderr.flush()
    keep = os.dup(2)
    try:
        with tempfile.TemporaryFile() as f:
            os.dup2(f.fileno(), 2)
            try:
                ctx, cam = make_ctx(cfg, surfaces)
                ctx.render(cam, params)
                ctx.readback()
                ctx.close()
            finally:
                os.dup2(keep, 2)
            f.seek(0)
            m = _POOLS.search(f.read().decode("utf-8", "replace"))
    finally:
        os.close(keep)
        if saved is None:
            os.environ.pop("RWR_WF_STATS", None)
        else:
            os.environ["RWR_WF_STATS"] = saved
    return (int(m.group(2)), int(m.group(4))) if m else (0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--sky", action="store_true", help="both arms with RWR_FLAG_SKY: the trace kernels' SKY forms")
    args = ap.parse_args()
    spheres, mesh = (("sphere", 0), ("sphere", 1)), (("part", 0),)
    side = dict(bench.CONFIGS["cfg3"], camera=dict(eye=(3.2, 1.4, -1.2), target=(0.2, 0.2, -2.2)))
    front = bench.CONFIGS["cfg3"]
    work = (("1080p suzanne, reference camera (no glossy hit), spheres glossy", front, 1, 4, spheres),
            ("1080p suzanne, reference camera (no glossy hit), spheres glossy", front, 16, 4, spheres),
            ("1080p suzanne from the side, spheres glossy", side, 1, 4, spheres), ("1080p suzanne from the side, spheres glossy", side, 16, 4, spheres),
            ("configs[3] 4K x16, mesh glossy", bench.CONFIGS["cfg4"], 16, 4, mesh))
    for name, cfg, spp, bounces, surfaces in work:
        deep = (rwr.FLAG_MULTI_BOUNCE if bounces > 1 else 0) | (rwr.FLAG_SKY if args.sky else 0)
        plain = rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep)
        if args.plain_only:
            ctx, cam = make_ctx(cfg, ())
            call_a = ctx.render_call(cam, plain)
            a = [time_frames(ctx, call_a, args.frames) for _ in range(args.repeats)]
            print(json.dumps(dict(workload=name, spp=spp, bounces=bounces, plain_ms=round(float(np.mean(a)), 4),
                                  spread=[round(min(a), 4), round(max(a), 4)])), flush=True)
            ctx.close()
            continue
        ctx, cam = make_ctx(cfg, surfaces)
        gloss = rwr.make_params(spp=spp, max_bounces=bounces, seed=3, flags=deep | rwr.FLAG_GLOSSY)
        call_a, call_b = ctx.render_call(cam, plain), ctx.render_call(cam, gloss)
        # on the way: the gloss changes the frame, and the primary rays are the same rays
        call_a()
        off, rays_off = ctx.readback()["color"], ctx.last_render_stats()
        call_b()
        on, rays_on, glossy = ctx.readback()["color"], ctx.last_render_stats(), ctx.last_gloss_stats()
        a, b = [], []
        for _ in range(args.repeats):
            a.append(time_frames(ctx, call_a, args.frames))
            b.append(time_frames(ctx, call_b, args.frames))
        ctx.close()
        pk_off, ln_off = packet_share(cfg, surfaces, plain)
        pk_on, ln_on = packet_share(cfg, surfaces, gloss)
        print(json.dumps(dict(workload=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=bounces, sky=bool(args.sky), frames_in_flight=2,
                              frames=args.frames, repeats=args.repeats, frame_changed=bool((on != off).any()),
                              same_primary_rays=bool(rays_on[0] == rays_off[0]), bounce_rays_plain=int(rays_off[1]), bounce_rays_gloss=int(rays_on[1]), glossy_rays=int(glossy),
                              packet_share_plain=round(pk_off / max(1, pk_off + ln_off), 4), packet_share_gloss=round(pk_on / max(1, pk_on + ln_on), 4),
                              plain_ms=round(float(np.mean(a)), 4), plain_spread=[round(min(a), 4), round(max(a), 4)],
                              gloss_ms=round(float(np.mean(b)), 4), gloss_spread=[round(min(b), 4), round(max(b), 4)],
                              gloss_minus_plain_us=round((float(np.mean(b)) - float(np.mean(a))) * 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
