"""What the time statistics cost (FS3D_OPT_TIME_STATS, FS3D_OPT_OUTPUT_SOURCE; csrc/kernels_stats.hip): the bench.py case, 256^3 fp32, one GPU.

  python tools/time_stats_cost.py --parent-lib DIR/libfs3d_hip.so [--out FILE]        -> profiles/time_stats_cost.txt

(a) mode 0 is not slower.  `python bench.py --gpus 1 --steps 20 --warmup 3` in fresh processes, one library per process (FS3D_LIB_PATH),
    `--rounds` rounds with the parent's library first, then as many with this tree's first.  Verdict, set before the run (DESIGN
    section 2): the median of this tree's process values is no lower than the smallest of the parent's.
(b) the step time per mode.  Children of this tool on this tree's library, one mode per fresh process, the modes 0, 1, 2 in turn and
    `--rounds` rounds: bench.py's loop (UpdateBoundaries + TimeStep, the error every 10th step), 3 warm-up steps, then `--repeats`
    timed blocks of 20 steps (host clock, synchronised); a process reports the median of its blocks.
(c) the kernels.  One child per mode 1, 2 under `rocprofv3 --kernel-trace` (alone: no counters, no other tracing): the device
    duration of every accumulation (k_time_stats_v4) and of one statistic layer per source (k_time_stats_layer) from the trace's
    timestamps, beside the bytes the rule says they move -- accumulation 54 (mode 2: 86) B per cell: 2 B of code, 16 B of `cur`, and
    4 + 32 (+ 32) B read and written back; layer: 4 + 32 (+ 32) B of sums read, 16 B written -- as a rate and as a share of the
    5.3 - 5.8 TB/s a copy reaches on this card.  (The trace, as in tools/output_filter_cost.py: the accumulation is
    enqueued inside the time step, where the tool cannot put events of its own around it, and the nine event classes of
    fs3d_enable_timing are the reference Profiler's names.)
(d) a kernel variant.  `--tree-lib FILE --skip-bench --note TEXT` runs (b) and (c) on another build of this tree's sources: how the
    nontemporal accumulator accesses were set against the plain ones the tree keeps (profiles/time_stats_cost.txt says how that
    build was made).
Every GPU child runs under its own `timeout`; the tool stops at the first child that fails.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "profiles", "time_stats_cost.txt")
N, STEPS, WARMUP = 256, 20, 3
COPY_TBS = (5.3, 5.8)


def run_child(cmd, env, seconds):
    """A GPU child under its own time limit; the first failure ends the tool."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("time_stats_cost: %s ended with status %d\n%s" % (" ".join(cmd), r.returncode, (r.stdout + r.stderr)[-2000:]))
    return r.stdout


def child(mode, repeats, layers):
    """bench.py's case and loop with FS3D_OPT_TIME_STATS = mode; prints one JSON line"""
    import bench
    from cmc_fluid_solver_amd import capi, grids
    dtype = np.float32
    g = grids.box(N, h=1.0 / (N - 1))
    s = capi.Solver(g, capi.fluid_params(dtype, bench.RE, bench.PR, bench.LAMBDA), dtype)
    s.set_option(capi.OPT_TIME_STATS, mode)

    def step(i):
        if i % 10 == 0:
            s.UpdateBoundaries()
            s.TimeStep(0.1, bench.NUM_GLOBAL, bench.NUM_LOCAL, True)
        else:
            s.time_step_async(0.1, bench.NUM_GLOBAL, bench.NUM_LOCAL)
    for i in range(WARMUP):
        step(i)
    s.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for i in range(STEPS):
            step(i)
        s.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    out = {"mode": mode, "ms_per_step": ms, "cells": N ** 3, "kernels": s.last_sweep_kernels()}
    if layers and mode:
        od = (54, 54, 52)
        rec = {}
        for source in ((0, 1, 2, 3) if mode == 2 else (0, 1, 3)):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            t = []
            for _ in range(WARMUP + repeats):
                t0 = time.perf_counter()
                s.GetLayer(od)
                t.append((time.perf_counter() - t0) * 1e3)
            rec[str(source)] = t[WARMUP:]
        out["record_ms"] = rec
    s.close()
    print(json.dumps(out))


def durations(path, name):
    rows = [r for r in csv.DictReader(open(path)) if name in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]


def rate_text(nbytes, us):
    tbs = nbytes / (us * 1e-6) / 1e12
    return "%.2f TB/s, %.0f - %.0f %% of the copy rate" % (tbs, 100 * tbs / COPY_TBS[1], 100 * tbs / COPY_TBS[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=None, help="internal: run one mode in this process")
    ap.add_argument("--layers", action="store_true", help="internal: the child also takes records of every source")
    ap.add_argument("--parent-lib", default=None, help="libfs3d_hip.so of the parent commit's build")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-lib", default=None, help="a build of this tree's sources to measure in place of the tree's own library (a kernel variant)")
    ap.add_argument("--skip-bench", action="store_true", help="leave out (a)")
    ap.add_argument("--note", default="", help="a line for the head of the file (which build this is)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.repeats, a.layers)
    lines = ["time statistics, %d^3 fp32 box (the bench.py case), one MI355X; tools/time_stats_cost.py" % N]
    if a.note:
        lines.append(a.note)

    def say(text):
        print(text, flush=True)
        lines.append(text)
    env0 = dict(os.environ)
    env0.pop("FS3D_LIB_PATH", None)
    if a.tree_lib:
        env0["FS3D_LIB_PATH"] = os.path.abspath(a.tree_lib)
        say("this tree's side: " + a.tree_lib)
    me = [sys.executable, os.path.abspath(__file__)]
    if not a.skip_bench:
        if not a.parent_lib or not os.path.isfile(a.parent_lib):
            raise SystemExit("time_stats_cost: --parent-lib: the library of the build to compare with (or --skip-bench)")
        val = {"parent": [], "this_tree": []}
        for order in (("parent", "this_tree"), ("this_tree", "parent")):
            for _ in range(a.rounds):
                for name in order:
                    env = dict(env0)
                    if name == "parent":
                        env["FS3D_LIB_PATH"] = os.path.abspath(a.parent_lib)
                    out = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)], env, 300)
                    val[name].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
                    print("    bench.py, %s: %.1f" % (name, val[name][-1]), file=sys.stderr, flush=True)
        tree, low = statistics.median(val["this_tree"]), min(val["parent"])
        say("(a) mode 0, python bench.py, Mcells/s, fresh processes alternating (%d rounds parent first, %d this tree first)" % (a.rounds, a.rounds))
        say("    parent:    " + ", ".join("%.1f" % v for v in val["parent"]))
        say("    this tree: " + ", ".join("%.1f" % v for v in val["this_tree"]))
        say("    median of this tree %.1f, smallest of the parent %.1f: %s" % (tree, low, "PASS" if tree >= low else "FAIL"))
    med = {0: [], 1: [], 2: []}
    rec = {}
    for rnd in range(a.rounds):
        for mode in (0, 1, 2):
            o = json.loads(run_child(me + ["--child", str(mode), "--repeats", str(a.repeats)] + (["--layers"] if rnd == 0 else []), env0, 300).strip().splitlines()[-1])
            med[mode].append(statistics.median(o["ms_per_step"]))
            print("    mode %d: %.4f ms per step" % (mode, med[mode][-1]), file=sys.stderr, flush=True)
            if "record_ms" in o:
                rec[mode] = o["record_ms"]
    say("(b) ms per step (host clock, %d-step blocks, process medians of %d blocks; %d processes per mode)" % (STEPS, a.repeats, a.rounds))
    for mode in (0, 1, 2):
        say("    mode %d: %s; median %.4f (+%.4f over mode 0)" % (mode, ", ".join("%.4f" % v for v in med[mode]), statistics.median(med[mode]),
                                                                statistics.median(med[mode]) - statistics.median(med[0])))
    say("(c) device time of the kernels (rocprofv3 --kernel-trace), median (min - max) us")
    cells = N ** 3
    for mode in (1, 2):
        tmp = tempfile.mkdtemp(prefix="time_stats_cost_")
        run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me + ["--child", str(mode), "--repeats", "1", "--layers"], env0, 600)
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
        if len(found) != 1:
            raise SystemExit("time_stats_cost: no kernel trace under " + tmp)
        acc = durations(found[0], "k_time_stats_v")[WARMUP:]          # either launch form; one launch per step, the warm-up steps first
        lay = durations(found[0], "k_time_stats_layer")
        if not acc or not lay:
            raise SystemExit("time_stats_cost: %d accumulations and %d layers in the trace of mode %d" % (len(acc), len(lay), mode))
        nb = (54 if mode == 1 else 86) * cells
        say("    mode %d accumulation k_time_stats_v4 / _v1: %.1f (%.1f - %.1f) us over %d launches; %d B/cell: %s"
            % (mode, statistics.median(acc), min(acc), max(acc), len(acc), nb // cells, rate_text(nb, statistics.median(acc))))
        say("    mode %d statistic layer k_time_stats_layer: %.1f (%.1f - %.1f) us over %d launches (not tuned)"
            % (mode, statistics.median(lay), min(lay), max(lay), len(lay)))
    for mode in sorted(rec):
        say("    mode %d record at 54 x 54 x 52 (fs3d_get_layer, returns synchronised), host clock ms per source: %s"
            % (mode, "; ".join("%s: %.3f" % (k, statistics.median(v)) for k, v in sorted(rec[mode].items()))))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
