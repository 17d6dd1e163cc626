#!/usr/bin/env python3
"""Cost and worth of multiple importance sampling for the light rays (RWR_FLAG_LIGHT_MIS, DESIGN §6 Cost) on the two worst cases the
record keeps for RWR_FLAG_LIGHT_PARTS - the whole mesh (part 0) emits, so every receiver touches an emitter: 1080p suzanne at 16 spp
with 2 bounces, configs[3]'s 4K x16 grid at 16 spp with 1 bounce (tools/light_probe.py's cases).  Three arms alternated in one process
(a block of frames of each, --repeats times), 2 frames in flight, tools/part_light_probe.py's protocol: the frame with
RWR_FLAG_EMISSIVE alone ("plain"), with RWR_FLAG_LIGHT_PARTS on top ("parts"), with RWR_FLAG_LIGHT_MIS on top of that ("mis").
One JSON line per case: mean and spread (min..max over the repeats) of every arm, the two ratios to the plain arm, the counts of both
flagged frames (they must be equal but for the emissive hits), and the equal-time error: against a long accumulation of the PLAIN
frame (--truth samples; no capped term darkens it), either flagged frame at spp S and the plain frame at the spp that takes the same
time.

--others times the frames that must not pay and touches no entry point or flag of the feature, so that a library without it
(RWR_HIP_LIB, a build of the parent commit) can run it too: RWR_FLAG_EMISSIVE alone with the emitting mesh, RWR_FLAG_LIGHT_PARTS on
top, and RWR_FLAG_LIGHT_SAMPLING with an emitting sphere.  Alternate the two libraries' runs in one session.

--forms times, the same way and as runnable on the parent's library, frames WITHOUT any light flag that run the GLOW forms of the trace
kernels which reserve more scratch or spill more vector registers than the parent's (profiles/mis_kernel_resources.txt): the emitting
mesh under RWR_FLAG_EMISSIVE + RWR_FLAG_SKY at 2 bounces (an EMIT generation and a last one), alone, with shadow rays, with the mesh a
mirror (SURF 1) and with the mesh glass (SURF 2), under the default schedule and under forced packets.  Per arm it also prints the trace
pools, rays and launches of one frame per kernel (RWR_WF_STATS), so that the record says which kernel ran."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from light_probe import LE, cases  # noqa: E402
from part_light_probe import PART_LE, frame  # noqa: E402
from soft_shadow_probe import make_ctx, stats, time_frames  # noqa: E402

LIGHT_PARTS, LIGHT_SAMPLING, LIGHT_MIS = 1 << 21, 1 << 16, 1 << 22


def params(rwr, spp, b, seed=3, extra=0):
    return rwr.make_params(spp=spp, max_bounces=b, seed=seed, flags=(rwr.FLAG_MULTI_BOUNCE if b > 1 else 0) | rwr.FLAG_EMISSIVE | extra)


def others(rwr, args):
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        out = dict(case=name, spp=spp, bounces=b, frames=args.frames, repeats=args.repeats, library=os.environ.get("RWR_HIP_LIB", "this build"))
        glow, parts, sphere = (ctx.render_call(cam, params(rwr, spp, b, extra=x)) for x in (0, LIGHT_PARTS, LIGHT_SAMPLING))
        arms = {"part_emissive": [], "part_light_parts": [], "sphere_light_sampling": []}
        for _ in range(args.repeats):
            ctx.set_sphere_emission(0, None)
            ctx.set_part_emission(0, PART_LE)
            arms["part_emissive"].append(time_frames(ctx, glow, args.frames))
            arms["part_light_parts"].append(time_frames(ctx, parts, args.frames))
            ctx.set_part_emission(0, None)
            ctx.set_sphere_emission(0, LE)
            arms["sphere_light_sampling"].append(time_frames(ctx, sphere, args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        print(json.dumps(out), flush=True)
        ctx.close()


FORCED = {"RWR_WF_GROUP": "5", "RWR_WF_PACKET_FILL": "0", "RWR_WF_PACKET_EXTENT": "1e30", "RWR_WF_MIN_PACKET_POOLS": "0"}   # tests/path_cases.py FORCED_SCHEDULE
_STATS = re.compile(r"rwr wavefront pools: packets (\d+) pools / (\d+) rays, per-lane (\d+) pools / (\d+) rays.*\n"
                    r"rwr wavefront launches: packet (\d+), per-lane (\d+), per-lane wide (\d+)")


def launches_of(rwr, cfg, setup, p):
    """One frame in a context of its own, which prints its pools and trace launches when it closes (RWR_WF_STATS): pools and rays that
    went to the packet kernel and to the per-lane kernel, launches of the packet, per-lane and wide per-lane kernels."""
    with tempfile.TemporaryFile() as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            ctx, cam = make_ctx(rwr, cfg)
            setup(ctx)
            ctx.render(cam, p)
            ctx.readback()
            ctx.close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        m = _STATS.findall(f.read().decode(errors="replace"))
    keys = ("packet_pools", "packet_rays", "lane_pools", "lane_rays", "packet_launches", "lane_launches", "wide_launches")
    return dict(zip(keys, (int(v) for v in m[-1]))) if m else None


def forms(rwr, args):
    os.environ["RWR_WF_STATS"] = "1"
    mirror, glass, sky, shadows = rwr.FLAG_MIRRORS, rwr.FLAG_GLASS, rwr.FLAG_SKY, rwr.FLAG_SHADOWS   # (flags the parent's library knows)
    arms = {"sky": (sky, lambda c: c.set_part_mirror(0, None)),
            "sky_shadows": (sky | shadows, lambda c: c.set_part_mirror(0, None)),
            "sky_mirror": (sky | mirror, lambda c: c.set_part_mirror(0, (0.9, 0.9, 0.9))),
            "sky_glass": (sky | glass, lambda c: c.set_part_glass(0, 1.5, (1.0, 1.0, 1.0)))}
    for schedule, env in (("default", {}), ("forced packets", FORCED)):
        os.environ.update(env)
        for name, cfg, spp, b in cases():
            b = max(b, 2)
            out = dict(case=name, schedule=schedule, spp=spp, bounces=b, frames=args.frames, repeats=args.repeats,
                       library=os.environ.get("RWR_HIP_LIB", "this build"))
            calls = {}
            ctx, cam = make_ctx(rwr, cfg)
            ctx.set_part_emission(0, PART_LE)
            for k, (x, setup) in arms.items():
                def emit_and(c, setup=setup):
                    c.set_part_emission(0, PART_LE)
                    setup(c)
                out["ran_" + k] = launches_of(rwr, cfg, emit_and, params(rwr, spp, b, extra=x))
                calls[k] = ctx.render_call(cam, params(rwr, spp, b, extra=x))
            times = {k: [] for k in arms}
            for _ in range(args.repeats):
                for k, (x, setup) in arms.items():
                    setup(ctx)
                    times[k].append(time_frames(ctx, calls[k], args.frames))
            for k, v in times.items():
                out[k] = stats(v)
            print(json.dumps(out), flush=True)
            ctx.close()
        for k in env:
            os.environ.pop(k, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--truth", type=int, default=2048, help="samples of the accumulation the errors are taken against")
    ap.add_argument("--others", action="store_true")
    ap.add_argument("--forms", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    rwr = graft.load_package()
    if args.others:
        return others(rwr, args)
    if args.forms:
        return forms(rwr, args)
    for name, cfg, spp, b in cases():
        ctx, cam = make_ctx(rwr, cfg)
        ctx.set_part_emission(0, PART_LE)
        flags = {"plain": 0, "parts": rwr.FLAG_LIGHT_PARTS, "mis": rwr.FLAG_LIGHT_PARTS | rwr.FLAG_LIGHT_MIS}
        calls = {k: ctx.render_call(cam, params(rwr, spp, b, extra=x)) for k, x in flags.items()}
        out = dict(case=name, width=cfg["width"], height=cfg["height"], spp=spp, bounces=b, frames_in_flight=2, frames=args.frames, repeats=args.repeats)
        for k in ("parts", "mis", "plain"):
            calls[k]()
            ctx.readback()
            out["counts_" + k] = dict(light=ctx.last_light_stats(), part=ctx.last_part_light_stats(), emissive_hits=ctx.last_emission_stats())
        arms = {k: [] for k in flags}
        for _ in range(args.repeats):
            for k in flags:
                arms[k].append(time_frames(ctx, calls[k], args.frames))
        for k, v in arms.items():
            out[k] = stats(v)
        ratio = {k: float(np.mean(arms[k]) / np.mean(arms["plain"])) for k in ("parts", "mis")}
        out.update(parts_over_plain=round(ratio["parts"], 4), mis_over_plain=round(ratio["mis"], 4), mis_over_parts=round(ratio["mis"] / ratio["parts"], 4))
        # equal time: a flagged frame at spp against the plain frame at round(spp x ratio); the truth: an accumulation of the plain frame
        ctx.set_frames_in_flight(1)
        ctx.accum_reset()
        aux = rwr.FLAG_AUX_OUTPUTS   # (the f32 colour plane is read back)
        acc = params(rwr, 64, b, seed=101, extra=rwr.FLAG_ACCUMULATE | aux)
        for _ in range(max(1, args.truth // 64)):
            ctx.render(cam, acc)
        truth = ctx.readback(aux=True)["color_f32"][..., :3].astype(np.float64)
        ctx.accum_reset()
        mse = lambda s, x: float(((frame(ctx, cam, params(rwr, s, b, extra=x | aux)) - truth) ** 2).mean())
        out.update(truth_samples=max(1, args.truth // 64) * 64, mse_plain_same_spp=mse(spp, 0))
        for k in ("parts", "mis"):
            spp_plain = max(spp, int(round(spp * ratio[k])))
            m, m_plain = mse(spp, flags[k]), mse(spp_plain, 0)
            out.update({"mse_" + k: m, "equal_time_spp_plain_" + k: spp_plain, "mse_plain_equal_time_" + k: m_plain,
                        "mse_ratio_equal_time_" + k: round(m / m_plain, 4) if m_plain else None})
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
