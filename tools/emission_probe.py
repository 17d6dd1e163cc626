#!/usr/bin/env python3
"""Cost of emissive surfaces (RWR_FLAG_EMISSIVE, DESIGN §6 Cost): ms per frame of a frame without the flag against the SAME frame with
the flag and one emitting part, and with one emitting sphere, alternated in one process (a block of plain frames, a block of each
emissive arm, --repeats times), 2 frames in flight, tools/soft_shadow_probe.py's protocol, on two large cases:
  1080p suzanne at 16 spp with 2 bounces, configs[3]'s 4K x16 grid at 16 spp with 1 bounce.
One JSON line per case: mean and spread (min..max over the repeats) of every arm, the ratios, the emissive hits of each arm.

--plain-only times the plain frame alone and touches no entry point of the feature: what a library without it (RWR_HIP_LIB, a build
of the parent commit) can run - the figure to hold against this build's plain arm: the flag must cost nothing where it is off.
Alternate the two libraries' runs in one session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from soft_shadow_probe import make_ctx, stats, time_frames  # noqa: E402  (the protocol's three steps: tools/ is a script's own directory)

LE = (8.0, 7.0, 5.0)


def cases():
    import bench
    return (("1080p suzanne spp 16 B 2", bench.CONFIGS["cfg3"], 16, 2), ("configs[3] 4K x16 spp 16 B 1", bench.CONFIGS["cfg4"], 16, 1))


def params(rwr, spp, b, emissive):
    flags = (rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | (rwr.FLAG_EMISSIVE if emissive else 0)
    return rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        plain = ctx.render_call(cam, params(rwr, spp, b, False))
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats,
                   library=os.environ.get("RWR_HIP_LIB") or "this build")
        if args.plain_only:
            out["plain"] = stats([time_frames(ctx, plain, args.frames) for _ in range(args.repeats)])
        else:
            glow = ctx.render_call(cam, params(rwr, spp, b, True))

            def arm(which):   # one emitter at a time: part 0 (the mesh), or sphere 0
                ctx.set_part_emission(0, LE if which == "part" else None)
                ctx.set_sphere_emission(0, LE if which == "sphere" else None)

            arms = {"plain": [], "part": [], "sphere": []}
            for which in ("part", "sphere"):
                arm(which)
                glow()
                ctx.readback()
                out[f"emissive_hits_{which}"] = ctx.last_emission_stats()
            for _ in range(args.repeats):
                arm(None)
                arms["plain"].append(time_frames(ctx, plain, args.frames))
                for which in ("part", "sphere"):
                    arm(which)
                    arms[which].append(time_frames(ctx, glow, args.frames))
            arm(None)
            for k, v in arms.items():
                out[k] = stats(v)
            for which in ("part", "sphere"):
                out[f"{which}_over_plain"] = round(float(np.mean(arms[which]) / np.mean(arms["plain"])), 4)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
