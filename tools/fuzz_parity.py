"""Fuzz against the CPU oracle for a given time (needs a GPU; the oracle is the checker here exactly as in tests/).
    python tools/fuzz_parity.py [--far] [seed] [seconds]    see tests/fuzz_common.py for what a frame is
--far: every scene moved up to 1e5 from the world origin, and every primary frame also rendered without AUX outputs.
    python tools/fuzz_parity.py --rest [seed] [seconds]     see tests/rest_common.py
--rest: lists of cases (seed, seed + 1, ...) each held at rest for 2 n + 2 frames on a context whose slots are modelled, so that
the frames compared with the oracle are served from the slot's kept records and ray plane.
    python tools/fuzz_parity.py --path [first] [count] [seconds]      see tests/path_cases.py
--path: path_cases.case(i) for i in [first, first + count) (default: the 64 cases after the committed list; a new context every
256 cases) against the tests' CPU reference of the extensions taken together (mirror_ref.c), with the tests' own comparison; with
seconds, the walk ends early once that time is up and says how far it came.
    python tools/fuzz_parity.py --path --glass [first] [count] [seconds]      see tests/glass_cases.py
--path --glass: glass_cases.glass_case(g) for g in [first, first + count) (default: the 64 cases after the committed list) against
glass_ref.c with glass_cases.compare, the three glass event counts included; the cases of glass_cases.ROUNDED_THROUGHPUT against
the reference that rounds the throughput to unorm16 (glass_cases.compare_rounded); the walk stops at the first mismatch.
    python tools/fuzz_parity.py --path --gloss [first] [count] [seconds]      see tests/gloss_cases.py
--path --gloss: gloss_cases.gloss_case(q) for q in [first, first + count) (default: the 64 cases after the committed 96) against
gloss_ref.c with gloss_cases.compare, the glossy-ray count and the three glass event counts included; otherwise as --glass (the
cases of gloss_cases.ROUNDED_THROUGHPUT, the first mismatch, the error against the rounded reference where it stops), and the last
line also gives the worst case's error against the rounded reference.
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
path = "--path" in sys.argv[1:]
gloss = "--gloss" in sys.argv[1:]
glass = "--glass" in sys.argv[1:] or gloss      # the gloss walk is the glass walk over another list, with one more count
args = [a for a in sys.argv[1:] if a not in ("--far", "--rest", "--path", "--glass", "--gloss")]
if glass and not path:
    sys.exit("--glass and --gloss go with --path")
if path:
    import tempfile

    import path_cases

    class _Tmp:   # the references' lib() builds into a directory from pytest's factory; here one of our own
        @staticmethod
        def mktemp(name):
            return tempfile.mkdtemp(prefix=name)

    if gloss:
        import gloss_cases as cases
        import gloss_ref

        L, make, n_listed, what = gloss_ref.lib(_Tmp), cases.gloss_case, cases.N_GLOSS_CASES, "gloss"
    elif glass:   # the list, its reference, its comparison; the glass walk stops at the first mismatch
        import glass_cases as cases
        import glass_ref

        L, make, n_listed, what = glass_ref.lib(_Tmp), cases.glass_case, cases.N_GLASS_CASES, "glass"
    else:
        import mirror_ref

        cases = path_cases
        L, make, n_listed, what = mirror_ref.lib(_Tmp), cases.case, cases.N_CASES, "path"
    meshes = {n: ref_loader.load_model_compute(r.RES_DIR, n + ".obj") for n in ("suzanne_lowpoly", "cube")}
    first = int(args[0]) if len(args) > 0 else n_listed
    count = int(args[1]) if len(args) > 1 else 64
    t_end = time.time() + float(args[2]) if len(args) > 2 else None
    worst = worst_ratio = worst_rounded = 0.0
    at = None
    t0 = time.time()
    done, failed, ctx, with_events, events, with_glossy, glossy = 0, [], None, 0, [0, 0, 0], 0, 0
    for i in range(first, first + count):
        if t_end is not None and time.time() >= t_end:
            break
        if done % 256 == 0:
            if ctx is not None:
                ctx.close()
            ctx = r.Context(0)
        c = make(i, ref_loader, orc, meshes["cube"], meshes["suzanne_lowpoly"])
        got = None
        try:
            got = cases.gpu_frame(r, c, ctx)
            if glass and i in cases.ROUNDED_THROUGHPUT:      # held to the reference that rounds the throughput, as the GPU test holds it
                err, against_plain = cases.compare_rounded(got, L, orc, c)
                print(f"{what} case {i}: colour error {against_plain:.3g} against the plain reference, {err:.3g} against the one that rounds the "
                      f"throughput to unorm16 ({err / path_cases.color_bar(c):.2f} of its bar)", flush=True)
            else:
                err = cases.compare(got, cases.reference(L, orc, c), c)
        except AssertionError as e:      # a mismatch is a finding: say which case (an error of the device is not caught)
            failed.append(i)
            print(f"MISMATCH at {what} case {i}: {e}", flush=True)
            if glass and got is None:
                break
            if glass:     # where it stops it also says what the reference that rounds the throughput would have said
                try:
                    err, _ = cases.compare_rounded(got, L, orc, c)
                    print(f"{what} case {i}: every integer equal; against the reference that rounds the throughput to unorm16 {err:.3g} "
                          f"({err / path_cases.color_bar(c):.2f} of its bar)", flush=True)
                except AssertionError as e2:
                    print(f"{what} case {i}: no match with the reference that rounds the throughput either: {e2}", flush=True)
                break
            err = 0.0
        if gloss and err / path_cases.color_bar(c) >= worst_ratio:      # the worst so far: what the rounded reference says of it
            worst_rounded = float(abs(got["color_f32"] - cases.reference(L, orc, c, thr_unorm16=True)["color_f32"]).max())
        cases.forget(c)
        if glass:
            with_events += sum(got["glass"]) > 0
            events = [a + b for a, b in zip(events, got["glass"])]
        if gloss:
            with_glossy += got["glossy"] > 0
            glossy += got["glossy"]
        if err / path_cases.color_bar(c) >= worst_ratio:
            worst, worst_ratio, at = err, err / path_cases.color_bar(c), i
        done += 1
        if done % 500 == 0:
            print(f"... {done} cases so far, {time.time() - t0:.0f} s, worst colour error {worst:.2e} (case {at}, {worst_ratio:.2f} of its bar)", flush=True)
    if ctx is not None:
        ctx.close()
    seen = f" {with_events} with glass events (reflected, transmitted, totally reflected: {tuple(events)})," if glass else ""
    if gloss:
        seen = f" {with_glossy} with glossy rays ({glossy} of them)," + seen
    print(f"{'ok' if not failed else 'FAILED ' + str(failed)}: {done} {what} cases ({first} ... {first + done - 1}) in {time.time() - t0:.0f} s,{seen} "
          f"worst colour error {worst:.2e} (case {at}, {worst_ratio:.2f} of its bar)" +
          (f", {worst_rounded:.2e} against the reference that rounds the throughput to unorm16" if gloss else ""))
    sys.exit(1 if failed else 0)
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
