#!/usr/bin/env python3
"""Cost of the Owen-scrambled Sobol sample sequence (RWR_FLAG_SOBOL, DESIGN §6 Cost): ms per frame of a frame without the flag against
the SAME frame with it, alternated in one process (a block of frames of each arm, --repeats times), 2 frames in flight,
tools/mis_probe.py's protocol, on three cases:
  1080p suzanne at 64 spp with 1 bounce (bench.py's cfg3), configs[3]'s 4K x16 grid at 16 spp with 1 bounce (cfg4), and a lamp-lit
  frame - 1080p suzanne, the mesh and sphere 0 emitting, 16 spp, 2 bounces, RWR_FLAG_LIGHT_SAMPLING + RWR_FLAG_LIGHT_PARTS +
  RWR_FLAG_LIGHT_MIS - where the light stage draws from the sequence too.
One JSON line per case: mean and spread (min..max over the repeats) of both arms, their ratio, and the ray counts of both frames.

--unflagged times bench.py's three wavefront configurations as bench.py renders them, without the flag, and touches no entry point or
flag of the feature, so that a library without it (RWR_HIP_LIB, a build of the parent commit) can run it too: the frames that must
not pay.  Alternate the two libraries' runs in one session; the bar is the parent's own spread between its runs."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from light_probe import LE  # noqa: E402
from part_light_probe import PART_LE  # noqa: E402
from soft_shadow_probe import make_ctx, stats, time_frames  # noqa: E402

SOBOL = 1 << 23


def cases(rwr):
    import bench
    lit = rwr.FLAG_EMISSIVE | rwr.FLAG_LIGHT_SAMPLING | rwr.FLAG_LIGHT_PARTS | rwr.FLAG_LIGHT_MIS
    return (("1080p suzanne spp 64 B 1", bench.CONFIGS["cfg3"], 64, 1, 0), ("configs[3] 4K x16 spp 16 B 1", bench.CONFIGS["cfg4"], 16, 1, 0),
            ("1080p suzanne lamp-lit spp 16 B 2, both light flags + MIS", bench.CONFIGS["cfg3"], 16, 2, lit))


def params(rwr, spp, b, extra=0):
    return rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=(rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | extra)


def unflagged(rwr, args):
    import bench
    for name in ("cfg3", "cfg4", "cfg5"):
        cfg = bench.CONFIGS[name]
        ctx, cam = make_ctx(rwr, cfg)
        ctx.set_frames_in_flight(3)     # (bench.py's setting for the wavefront configurations)
        call = ctx.render_call(cam, params(rwr, cfg["spp"], cfg["bounces"]))
        v = [time_frames(ctx, call, args.frames) for _ in range(args.repeats)]
        print(json.dumps(dict(config=name, spp=cfg["spp"], bounces=cfg["bounces"], frames=args.frames, repeats=args.repeats,
                              library=os.environ.get("RWR_HIP_LIB", "this build"), **stats(v))), flush=True)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--unflagged", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    if args.unflagged:
        return unflagged(rwr, args)
    for name, cfg, spp, b, extra in cases(rwr):
        ctx, cam = make_ctx(rwr, cfg)
        if extra:
            ctx.set_part_emission(0, PART_LE)
            ctx.set_sphere_emission(0, LE)
        calls = {"hashed": ctx.render_call(cam, params(rwr, spp, b, extra)), "sobol": ctx.render_call(cam, params(rwr, spp, b, extra | SOBOL))}
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats)
        for k, call in calls.items():
            call()
            ctx.readback()
            out["counts_" + k] = dict(render=ctx.last_render_stats(), light=ctx.last_light_stats())
        arms = {k: [] for k in calls}
        for _ in range(args.repeats):
            for k in calls:
                arms[k].append(time_frames(ctx, calls[k], args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        out["sobol_over_hashed"] = round(float(np.mean(arms["sobol"]) / np.mean(arms["hashed"])), 4)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
