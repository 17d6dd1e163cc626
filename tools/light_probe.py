#!/usr/bin/env python3
"""Cost and worth of light sampling (RWR_FLAG_LIGHT_SAMPLING, DESIGN §6 Cost): ms per frame of a frame with RWR_FLAG_EMISSIVE and one
emitting sphere against the SAME frame with the flag on top, alternated in one process (a block of plain frames, a block of flagged
frames, --repeats times), 2 frames in flight, tools/soft_shadow_probe.py's protocol, on two large cases:
  1080p suzanne at 16 spp with 2 bounces, configs[3]'s 4K x16 grid at 16 spp with 1 bounce.
One JSON line per case: mean and spread (min..max over the repeats) of either arm, the ratio, the three counts of the flagged frame,
and the equal-time error: the mean squared error, against a long accumulation of the flagged frame (--truth samples), of the flagged
frame at spp S and of the plain frame at the spp that takes the same time, S x the ratio rounded to a whole number."""
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


def params(rwr, spp, b, light, seed=3, extra=0):
    flags = (rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_EMISSIVE | (rwr.FLAG_LIGHT_SAMPLING if light else 0) | extra
    return rwr.make_params(spp=spp, max_bounces=b, seed=seed, flags=flags)


def frame(ctx, cam, p):
    ctx.render(cam, p)
    return ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--truth", type=int, default=2048, help="samples of the accumulation the errors are taken against")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        ctx.set_sphere_emission(0, LE)
        plain, light = ctx.render_call(cam, params(rwr, spp, b, False)), ctx.render_call(cam, params(rwr, spp, b, True))
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats)
        light()
        ctx.readback()
        out["light_rays"], out["reached"], out["suppressed_hits"] = ctx.last_light_stats()
        out["emissive_hits_light"] = ctx.last_emission_stats()
        plain()
        ctx.readback()
        out["emissive_hits_plain"] = ctx.last_emission_stats()
        arms = {"plain": [], "light": []}
        for _ in range(args.repeats):
            arms["plain"].append(time_frames(ctx, plain, args.frames))
            arms["light"].append(time_frames(ctx, light, args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        ratio = float(np.mean(arms["light"]) / np.mean(arms["plain"]))
        out["light_over_plain"] = round(ratio, 4)
        # equal time: the flagged frame at spp against the plain frame at round(spp x ratio); the truth: an accumulation of the flagged frame
        ctx.set_frames_in_flight(1)
        ctx.accum_reset()
        aux = rwr.FLAG_AUX_OUTPUTS   # (the f32 colour plane is read back)
        acc = params(rwr, 64, b, True, seed=101, extra=rwr.FLAG_ACCUMULATE | aux)
        for _ in range(max(1, args.truth // 64)):
            ctx.render(cam, acc)
        truth = ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)
        ctx.accum_reset()
        spp_plain = max(spp, int(round(spp * ratio)))
        mse_light = float(((frame(ctx, cam, params(rwr, spp, b, True, extra=aux)) - truth) ** 2).mean())
        mse_plain = float(((frame(ctx, cam, params(rwr, spp_plain, b, False, extra=aux)) - truth) ** 2).mean())
        mse_plain_same_spp = float(((frame(ctx, cam, params(rwr, spp, b, False, extra=aux)) - truth) ** 2).mean())
        out.update(truth_samples=max(1, args.truth // 64) * 64, equal_time_spp_plain=spp_plain, mse_light=mse_light, mse_plain_equal_time=mse_plain,
                   mse_plain_same_spp=mse_plain_same_spp, mse_ratio_equal_time=round(mse_light / mse_plain, 4) if mse_plain else None)
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
