"""Four-arm A/B of the benchmark on one GPU, arms interleaved run by run (the procedure of the r11 to r13 rounds):
  parent      a build of the parent commit, loaded through RWR_HIP_LIB
  change      this tree's library
  off         this tree's library with a knob switched off (KNOB=0)
  parent_off  the parent's library with the same knob switched off: what `off` must read as when the change lives behind the knob
Each round runs `bench.py`, `bench.py --config loop` and `bench.py --config cfg2b` in every arm.  Prints every ms_per_step in run
order, then min / median / max per config and arm and the verdict by the standing claim rule: every change run faster than every
parent run, and the ratio of medians beyond three times the parent's own max/min spread.

  python tools/ab3.py --parent-lib PATH --knob RWR_LEAN_REST [--rounds 4] [--configs cfg2,loop,cfg2b] [--out FILE]

A run that fails ends the script: nothing more is started on the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(arm, config, env_extra, bench_args, limit):
    env = dict(os.environ, **env_extra)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + ([] if config == "cfg2" else ["--config", config]) + bench_args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-2000:] + r.stderr[-2000:])
        raise SystemExit(f"{arm} {config}: bench.py ended with status {r.returncode}; stopping")
    return json.loads(r.stdout.strip().split("\n")[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--knob", required=True)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--configs", default="cfg2,loop,cfg2b")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one bench.py run may take")
    ap.add_argument("bench_args", nargs="*", help="passed on to bench.py (after --)")
    args = ap.parse_args()
    parent = {"RWR_HIP_LIB": os.path.abspath(args.parent_lib)}
    arms = [("parent", parent), ("change", {}), ("off", {args.knob: "0"}), ("parent_off", dict(parent, **{args.knob: "0"}))]
    configs = args.configs.split(",")
    lines, res = [], {}
    for _ in range(args.rounds):
        for config in configs:
            for arm, env in arms:
                ms = run(arm, config, env, args.bench_args, args.limit)
                res.setdefault((config, arm), []).append(ms)
                lines.append(f"{arm} {'cfg2' if config == 'cfg2' else '--config ' + config} {ms}")
                print(lines[-1], flush=True)
    lines.append("#")
    lines.append("# per config and arm: runs, min / median / max in us per frame")
    for config in configs:
        for arm, _ in arms:
            v = [1e3 * x for x in res[(config, arm)]]
            lines.append(f"# {config:<6} {arm:<10} n={len(v)}  {min(v):6.2f} / {statistics.median(v):6.2f} / {max(v):6.2f}")
        p, c, o, po = (res[(config, a)] for a in ("parent", "change", "off", "parent_off"))
        spread = max(p) / min(p)
        ratio = statistics.median(c) / statistics.median(p)
        all_faster = max(c) < min(p)
        claimed = all_faster and (1.0 - ratio) > 3.0 * (spread - 1.0)
        lines.append(f"# {config:<6} change / parent, ratio of medians: {ratio:.3f}   off / parent: {statistics.median(o) / statistics.median(p):.3f}   "
                     f"off / parent_off: {statistics.median(o) / statistics.median(po):.3f}   "
                     f"(parent's spread max/min: {spread:.3f}; {'every change run faster than every parent run' if all_faster else 'change runs NOT all faster than the parent runs'}; "
                     f"claim rule: {'met' if claimed else 'NOT met'})")
    print("\n".join(lines[len(lines) - 2 - (len(arms) + 1) * len(configs):]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
