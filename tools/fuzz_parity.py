"""Fuzz against the CPU oracle for a given time (needs a GPU; the oracle is the checker here exactly as in tests/).
    python tools/fuzz_parity.py [--far] [seed] [seconds]    see tests/fuzz_common.py for what a frame is
--far: every scene moved up to 1e5 from the world origin, and every primary frame also rendered without AUX outputs.
    python tools/fuzz_parity.py --rest [seed] [seconds]     see tests/rest_common.py
--rest: lists of cases (seed, seed + 1, ...) each held at rest for 2 n + 2 frames on a context whose slots are modelled, so that
the frames compared with the oracle are served from the slot's kept records and ray plane.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import __graft_entry__ as g
from oracle import oracle as orc, ref_loader
import fuzz_common

r = g.load_package()
far = "--far" in sys.argv[1:]
rest = "--rest" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a not in ("--far", "--rest")]
seed = int(args[0]) if len(args) > 0 else 1
seconds = float(args[1]) if len(args) > 1 else 30.0
if rest:
    import rest_common

    meshes = {n: ref_loader.load_model_compute(r.RES_DIR, n + ".obj") for n in ("suzanne_lowpoly", "cube")}
    meshes = {"suzanne": meshes["suzanne_lowpoly"], "cube": meshes["cube"]}
    t_end, n_cases = time.time() + seconds, 0
    with rest_common.tracked(r) as ctx:
        while time.time() < t_end:
            for c in rest_common.draw_cases(orc, ref_loader, meshes, seed):
                n = c["n_slots"]
                ctx.upload(c["model"]); ctx.set_spheres(c["spheres"]); ctx.resize(*c["size"]); ctx.set_slots(n)
                rest_common.rest(ctx, n, rest_common.Call(c["cam"]), rest_common.oracle_frame(orc, c["cam"], c["size"], c["spheres"], c["model"]),
                                 2 * n + 2, (seed, c["name"]))
                n_cases += 1
                if time.time() >= t_end:
                    break
            seed += 1
        print(f"ok: {n_cases} cases at rest, {ctx.frames} frames ({ctx.slots.served} loaded their rays, {ctx.slots.builds} planes built), "
              f"worst colour difference {ctx.worst:.2e}")
    sys.exit(0)
with r.Context(0) as ctx:
    n_frames, n_path, n_dormant, worst = fuzz_common.run(r, orc, ref_loader, ctx, seed, seconds, verbose=True,
                                                         many_samples=bool(int(os.environ.get("FUZZ_MANY_SAMPLES", "0"))), far=far, plain=far)
print(f"ok: {n_frames} frames ({n_path} path-traced, {n_dormant} with single triangles / orthographic rays), worst colour difference {worst:.2e}")
