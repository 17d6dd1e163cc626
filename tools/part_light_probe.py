#!/usr/bin/env python3
"""Cost and worth of light sampling towards emitting parts (RWR_FLAG_LIGHT_PARTS, DESIGN §6 Cost): ms per frame of a frame with
RWR_FLAG_EMISSIVE whose mesh (part 0) emits against the SAME frame with the flag on top, alternated in one process (a block of plain
frames, a block of flagged frames, --repeats times), 2 frames in flight, tools/light_probe.py's protocol and its two large cases:
  1080p suzanne at 16 spp with 2 bounces, configs[3]'s 4K x16 grid at 16 spp with 1 bounce.
One JSON line per case: mean and spread (min..max over the repeats) of either arm, the ratio, the flagged frame's counts (the stage's
totals and the mesh light's share, the list's length is the scene's face count), and the equal-time error as tools/light_probe.py
takes it: against a long accumulation of the flagged frame (--truth samples), the flagged frame at spp S and the plain frame at the
spp that takes the same time.

--others times the frames that must not pay and touches no entry point of the feature, so that a library without it (RWR_HIP_LIB, a
build of the parent commit) can run it too: RWR_FLAG_LIGHT_SAMPLING with an emitting sphere, RWR_FLAG_EMISSIVE alone with that sphere,
RWR_FLAG_EMISSIVE alone with the emitting mesh.  Alternate the two libraries' runs in one session."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from light_probe import LE, cases  # noqa: E402
from soft_shadow_probe import make_ctx, stats, time_frames  # noqa: E402

PART_LE = (0.5, 0.4, 0.3)


def params(rwr, spp, b, parts=False, light=False, seed=3, extra=0):
    flags = ((rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_EMISSIVE | (rwr.FLAG_LIGHT_PARTS if parts else 0) |
             (rwr.FLAG_LIGHT_SAMPLING if light else 0) | extra)
    return rwr.make_params(spp=spp, max_bounces=b, seed=seed, flags=flags)


def frame(ctx, cam, p):
    ctx.render(cam, p)
    return ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)


def others(rwr, args):
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        out = dict(case=name, spp=spp, bounces=b, frames=args.frames, repeats=args.repeats, library=os.environ.get("RWR_HIP_LIB", "this build"))
        sphere_glow = ctx.render_call(cam, params(rwr, spp, b))
        sphere_light = ctx.render_call(cam, rwr.make_params(spp=spp, max_bounces=b, seed=3, flags=(rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_EMISSIVE | (1 << 16)))
        arms = {"sphere_emissive": [], "sphere_light_sampling": [], "part_emissive": []}
        for _ in range(args.repeats):
            ctx.set_part_emission(0, None)
            ctx.set_sphere_emission(0, LE)
            arms["sphere_emissive"].append(time_frames(ctx, sphere_glow, args.frames))
            arms["sphere_light_sampling"].append(time_frames(ctx, sphere_light, args.frames))
            ctx.set_sphere_emission(0, None)
            ctx.set_part_emission(0, PART_LE)
            arms["part_emissive"].append(time_frames(ctx, sphere_glow, args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        print(json.dumps(out), flush=True)
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--truth", type=int, default=2048, help="samples of the accumulation the errors are taken against")
    ap.add_argument("--others", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    if args.others:
        return others(rwr, args)
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        ctx.set_part_emission(0, PART_LE)
        plain, parts = ctx.render_call(cam, params(rwr, spp, b)), ctx.render_call(cam, params(rwr, spp, b, parts=True))
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats)
        parts()
        ctx.readback()
        out["light_rays"], out["reached"], out["suppressed_hits"] = ctx.last_light_stats()
        out["part_light_rays"], out["part_reached"], out["part_suppressed_hits"] = ctx.last_part_light_stats()
        out["emissive_hits_parts"] = ctx.last_emission_stats()
        plain()
        ctx.readback()
        out["emissive_hits_plain"] = ctx.last_emission_stats()
        arms = {"plain": [], "parts": []}
        for _ in range(args.repeats):
            arms["plain"].append(time_frames(ctx, plain, args.frames))
            arms["parts"].append(time_frames(ctx, parts, args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        ratio = float(np.mean(arms["parts"]) / np.mean(arms["plain"]))
        out["parts_over_plain"] = round(ratio, 4)
        # equal time: the flagged frame at spp against the plain frame at round(spp x ratio); the truth: an accumulation of the flagged frame
        ctx.set_frames_in_flight(1)
        ctx.accum_reset()
        aux = rwr.FLAG_AUX_OUTPUTS   # (the f32 colour plane is read back)
        acc = params(rwr, 64, b, parts=True, seed=101, extra=rwr.FLAG_ACCUMULATE | aux)
        for _ in range(max(1, args.truth // 64)):
            ctx.render(cam, acc)
        truth = ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)
        ctx.accum_reset()
        spp_plain = max(spp, int(round(spp * ratio)))
        mse_parts = float(((frame(ctx, cam, params(rwr, spp, b, parts=True, extra=aux)) - truth) ** 2).mean())
        mse_plain = float(((frame(ctx, cam, params(rwr, spp_plain, b, extra=aux)) - truth) ** 2).mean())
        mse_plain_same_spp = float(((frame(ctx, cam, params(rwr, spp, b, extra=aux)) - truth) ** 2).mean())
        out.update(truth_samples=max(1, args.truth // 64) * 64, equal_time_spp_plain=spp_plain, mse_parts=mse_parts, mse_plain_equal_time=mse_plain,
                   mse_plain_same_spp=mse_plain_same_spp, mse_ratio_equal_time=round(mse_parts / mse_plain, 4) if mse_plain else None)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
