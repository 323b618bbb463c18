"""What the time statistics cost (FS3D_OPT_TIME_STATS, FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_TIME_STATS_EVERY, FS3D_OPT_OUTPUT_SOURCE;
csrc/kernels_stats.hip): the bench.py case, 256^3 fp32, one GPU.

  python tools/time_stats_cost.py --parent-lib DIR/libfs3d_hip.so --out profiles/time_stats_cross_cost.txt

(profiles/time_stats_cost.txt is the record of the commit that brought modes 1 and 2, written by this tool as it stood then: it counts
the bytes of every accumulator once, this tool counts what is read and what is written separately.)

The cases: mode 0, 1, 2, `2x` (mode 2 with the cross sums) and `2x/4` (the same with a stride of 4).
(a) mode 0 is not slower.  `python bench.py --gpus 1 --steps 20 --warmup 3` in fresh processes, one library per process (FS3D_LIB_PATH),
    `--rounds` rounds with the parent's library first, then as many with this tree's first.  Verdict, set before the run (DESIGN
    section 2): the median of this tree's process values is no lower than the smallest of the parent's.
(b) the step time per case.  Children of this tool on this tree's library, one case per fresh process, the cases in turn and
    `--rounds` rounds: bench.py's loop (UpdateBoundaries + TimeStep, the error every 10th step), 3 warm-up steps, then `--repeats`
    timed blocks of 20 steps (host clock, synchronised); a process reports the median of its blocks.
(c) the kernels.  Per case 1, 2, 2x `--rounds` children under `rocprofv3 --kernel-trace` (alone: no counters, no other tracing), and for
    the modes 1 and 2 as many on the parent's library, the two sides alternating and taking turns to go first, the launches of a side
    pooled (one process differs from the next by a few per cent with the same code: where its 9 to 19 arrays lie): the device duration of every accumulation (k_time_stats_v4) and of one statistic layer per
    source and moment (k_time_stats_layer) from the trace's timestamps, beside the bytes the rule says they move -- accumulation: 2 B of
    code and 16 B of `cur` read, 4 + 32 (mode 2: + 32, cross: + 48) B of counts and sums read and as many written, 90, 154 and 250 B per
    cell -- as a rate and as a share of the 5.3 - 5.8 TB/s a copy reaches on this card.  Verdicts, set before the
    run: modes 1 and 2, whose instantiations this tree left alone -- this tree's median is no higher than the parent's largest single
    launch; the cross kernel -- its rate is at least 0.9 times the mode 2 kernel's of the same session (twice the +-5 % box-to-box
    spread of the README).  (The trace, as in tools/output_filter_cost.py: the accumulation is enqueued inside the time step, where
    the tool cannot put events of its own around it, and the nine event classes of fs3d_enable_timing are the reference Profiler's
    names.)
(e) the gradient sums (FS3D_OPT_TIME_STATS_GRAD; k_time_grad).  `--gradients --out profiles/time_grad_cost.txt` runs (a), then (b) on the
    cases 0, 1, 1g, 2, 2g (g: with the gradient sums), then ONE child of case 1g under `rocprofv3 --kernel-trace` (alone): the median
    device time of k_time_grad<float> and of k_time_stats_v4<float, 1> over the same 20 steps.  The rule's bytes: the mode-1 kernel
    moves 54 B/cell counting every accumulator once (90 with reads and writes apart), the gradient kernel 42 when every field
    value is fetched once -- 2 of code, 4 of count, 12 of fields, 24 of sums -- (70 apart), so equal time leaves about 29 % for the
    neighbours' planes coming through the caches and for the arithmetic.  Verdict, set before the run: the median of k_time_grad is
    no larger than the median of the mode-1 kernel in that same trace.
(f) the wall sums (FS3D_OPT_TIME_STATS_WALL; k_time_wall).  `--wall --out profiles/wall_loads_cost.txt` runs, on the box and on the box
    with an obstacle, ONE child of case 1gw (mode 1 with the gradient sums and the wall sums) under `rocprofv3 --kernel-trace` (alone):
    the median device time of k_time_wall<float>, k_time_grad<float> and k_time_stats_v4<float, 1> over the same 20 steps, so the
    three kernels alternate step by step in one process; the fraction of carriers among the cells (from the numpy twin); and, in a
    child of its own, the time a plain read of a table of the code table's size takes (2 B per cell: torch's int16 sum under
    device events, back to back -- the table stays in the Infinity Cache -- and with a 1 GiB fill between the reads).  No verdict:
    nobody has measured this before.
(d) a kernel variant.  `--tree-lib FILE --skip-bench --note TEXT` runs (b) and (c) on another build of this tree's sources.
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
# case: (FS3D_OPT_TIME_STATS, FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_TIME_STATS_EVERY)
CASES = {"0": (0, 0, 1), "1": (1, 0, 1), "2": (2, 0, 1), "2x": (2, 1, 1), "2x/4": (2, 1, 4)}
# --gradients: the cases of (e); a trailing g sets FS3D_OPT_TIME_STATS_GRAD
GRAD_CASES = {"0": (0, 0, 1), "1": (1, 0, 1), "1g": (1, 0, 1), "2": (2, 0, 1), "2g": (2, 0, 1)}
# --wall: the case of (f), on both geometries
WALL_CASES = {"1gw": (1, 0, 1)}
GEOMETRIES = ("box", "obstacle")
GRAD_BYTES = 2 + 12 + 2 * (4 + 24)                           # code and fields read once, counts and sums read and written
# bytes per cell of one accumulation, fp32: code and `cur` read, counts and sums read and written
BYTES = {"1": 18 + 2 * 36, "2": 18 + 2 * 68, "2x": 18 + 2 * 116}
CROSS_RATE_SHARE = 0.9


def run_child(cmd, env, seconds):
    """A GPU child under its own time limit; the first failure ends the tool."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("time_stats_cost: %s ended with status %d\n%s" % (" ".join(cmd), r.returncode, (r.stdout + r.stderr)[-2000:]))
    return r.stdout


def geometry(name):
    from cmc_fluid_solver_amd import grids
    return grids.box(N, h=1.0 / (N - 1)) if name == "box" else grids.box_with_obstacle(N, h=1.0 / (N - 1))


def read_child(repeats):
    """(f): a plain read of 2 B per cell, us per read under device events; prints one JSON line"""
    import torch
    t = torch.ones(N ** 3, dtype=torch.int16, device="cuda")
    fill = torch.empty(1 << 28, dtype=torch.int32, device="cuda")
    out = {}
    for name in ("back to back", "after a 1 GiB fill"):
        us = []
        for i in range(WARMUP + repeats):
            if name != "back to back":
                fill.fill_(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.sum(dtype=torch.int32)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out[name] = us[WARMUP:]
    print(json.dumps(out))


def child(case, repeats, layers, geom="box"):
    """bench.py's case and loop with the options of `case`; prints one JSON line"""
    import bench
    from cmc_fluid_solver_amd import capi
    dtype = np.float32
    mode, cross, every = {**CASES, **GRAD_CASES, **WALL_CASES}[case]
    g = geometry(geom)
    s = capi.Solver(g, capi.fluid_params(dtype, bench.RE, bench.PR, bench.LAMBDA), dtype)
    s.set_option(capi.OPT_TIME_STATS, mode)
    if cross:                                                  # (a library of the parent commit knows neither option: cases 0, 1, 2 only)
        s.set_option(capi.OPT_TIME_STATS_CROSS, cross)
    if every != 1:
        s.set_option(capi.OPT_TIME_STATS_EVERY, every)
    if "g" in case:
        s.set_option(capi.OPT_TIME_STATS_GRAD, 1)
    if "w" in case:
        s.set_option(capi.OPT_TIME_STATS_WALL, 1)

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
    out = {"case": case, "ms_per_step": ms, "cells": N ** 3, "kernels": s.last_sweep_kernels()}
    if layers and mode and "g" not in case:
        od = (54, 54, 52)
        rec = {}
        sources = [(0, 0), (1, 0), (3, 0)] + ([(2, 0)] if mode == 2 else []) + ([(2, 1), (2, 2)] if cross else [])
        for source, moment in sorted(sources):
            s.set_option(capi.OPT_OUTPUT_SOURCE, source)
            if cross:
                s.set_option(capi.OPT_OUTPUT_MOMENT, moment)
            t = []
            for _ in range(WARMUP + repeats):
                t0 = time.perf_counter()
                s.GetLayer(od)
                t.append((time.perf_counter() - t0) * 1e3)
            rec["%d.%d" % (source, moment)] = t[WARMUP:]
        out["record_ms"] = rec
    s.close()
    print(json.dumps(out))


def durations(path, name):
    rows = [r for r in csv.DictReader(open(path)) if name in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]


def tbs(nbytes, us):
    return nbytes / (us * 1e-6) / 1e12


def rate_text(nbytes, us):
    r = tbs(nbytes, us)
    return "%.2f TB/s, %.0f - %.0f %% of the copy rate" % (r, 100 * r / COPY_TBS[1], 100 * r / COPY_TBS[0])


def traced(me, case, env):
    """One child of `case` under rocprofv3 --kernel-trace: (accumulation durations after the warm-up, layer durations), us"""
    tmp = tempfile.mkdtemp(prefix="time_stats_cost_")
    run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me + ["--child", case, "--repeats", "1", "--layers"], env, 600)
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
    if len(found) != 1:
        raise SystemExit("time_stats_cost: no kernel trace under " + tmp)
    acc = durations(found[0], "k_time_stats_v")[WARMUP:]              # either launch form; one launch per step, the warm-up steps first
    lay = durations(found[0], "k_time_stats_layer")
    if not acc or not lay:
        raise SystemExit("time_stats_cost: %d accumulations and %d layers in the trace of case %s" % (len(acc), len(lay), case))
    return acc, lay


def wall_cost(a):
    """(f) of the module docstring"""
    from cmc_fluid_solver_amd import layer_output as LO
    lines = ["wall sums (FS3D_OPT_TIME_STATS_WALL), %d^3 fp32, one MI355X; tools/time_stats_cost.py --wall" % N]
    if a.note:
        lines.append(a.note)

    def say(text):
        print(text, flush=True)
        lines.append(text)
    env0 = dict(os.environ)
    env0.pop("FS3D_LIB_PATH", None)
    me = [sys.executable, os.path.abspath(__file__)]
    cells = N ** 3
    say("device time over the same %d steps of one trace per geometry (rocprofv3 --kernel-trace, case 1gw: the three kernels run in every step), median (min - max) us" % STEPS)
    for geom in GEOMETRIES:
        ty = np.asarray(geometry(geom).type)
        ncar = int(np.logical_or.reduce(LO.exposed_faces(ty)).sum())
        nwall = int(((ty == 2) | (ty == 3)).sum())
        tmp = tempfile.mkdtemp(prefix="time_wall_cost_")
        run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me +
                  ["--child", "1gw", "--repeats", "1", "--geometry", geom], env0, 600)
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
        if len(found) != 1:
            raise SystemExit("time_stats_cost: no kernel trace under " + tmp)
        say("  %s: %d carriers among %d cells, a fraction of %.5f (%d wall cells)" % (geom, ncar, cells, ncar / cells, nwall))
        for name in ("k_time_wall<", "k_time_grad<", "k_time_stats_v4<float, 1>"):
            d = durations(found[0], name)[WARMUP:]
            if len(d) != STEPS:
                raise SystemExit("time_stats_cost: %d launches of %s in the trace, %d steps" % (len(d), name, STEPS))
            say("    %-28s %.1f (%.1f - %.1f) us per accumulated step" % (name.rstrip("<") + ":", statistics.median(d), min(d), max(d)))
    o = json.loads(run_child(me + ["--child", "read", "--repeats", str(max(a.repeats, 10))], env0, 300).strip().splitlines()[-1])
    say("a plain read of %d x 2 B (the size of the code table; torch int16 sum, device events), median (min - max) us" % cells)
    for name, us in o.items():
        say("    %-20s %.1f (%.1f - %.1f): %s" % (name + ":", statistics.median(us), min(us), max(us), rate_text(2 * cells, statistics.median(us))))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="internal: run one case in this process")
    ap.add_argument("--layers", action="store_true", help="internal: the child also takes records of every source")
    ap.add_argument("--parent-lib", default=None, help="libfs3d_hip.so of the parent commit's build")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tree-lib", default=None, help="a build of this tree's sources to measure in place of the tree's own library (a kernel variant)")
    ap.add_argument("--skip-bench", action="store_true", help="leave out (a) and the parent's side of (c)")
    ap.add_argument("--gradients", action="store_true", help="(e): the cost of FS3D_OPT_TIME_STATS_GRAD in place of (b) and (c)")
    ap.add_argument("--wall", action="store_true", help="(f): the cost of FS3D_OPT_TIME_STATS_WALL, alone: no (a), (b), (c)")
    ap.add_argument("--geometry", default="box", choices=GEOMETRIES, help="internal: the child's grid")
    ap.add_argument("--note", default="", help="a line for the head of the file (which build this is)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.child == "read":
        return read_child(a.repeats)
    if a.child is not None:
        return child(a.child, a.repeats, a.layers, a.geometry)
    if a.wall:
        return wall_cost(a)
    lines = ["time statistics, %d^3 fp32 box (the bench.py case), one MI355X; tools/time_stats_cost.py" % N,
             "bytes per cell count what an accumulation reads and what it writes separately: mode 1 %d, mode 2 %d, with the cross sums %d"
             % (BYTES["1"], BYTES["2"], BYTES["2x"]),
             "(profiles/time_stats_cost.txt, the record of the commit before, counts every accumulator once: 54 and 86)"]
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
    envp = None
    me = [sys.executable, os.path.abspath(__file__)]
    if not a.skip_bench:
        if not a.parent_lib or not os.path.isfile(a.parent_lib):
            raise SystemExit("time_stats_cost: --parent-lib: the library of the build to compare with (or --skip-bench)")
        envp = dict(env0)
        envp["FS3D_LIB_PATH"] = os.path.abspath(a.parent_lib)
        val = {"parent": [], "this_tree": []}
        for order in (("parent", "this_tree"), ("this_tree", "parent")):
            for _ in range(a.rounds):
                for name in order:
                    out = run_child([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)],
                                    envp if name == "parent" else env0, 300)
                    val[name].append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])
                    print("    bench.py, %s: %.1f" % (name, val[name][-1]), file=sys.stderr, flush=True)
        tree, low = statistics.median(val["this_tree"]), min(val["parent"])
        say("(a) mode 0, python bench.py, Mcells/s, fresh processes alternating (%d rounds parent first, %d this tree first)" % (a.rounds, a.rounds))
        say("    parent:    " + ", ".join("%.1f" % v for v in val["parent"]))
        say("    this tree: " + ", ".join("%.1f" % v for v in val["this_tree"]))
        say("    median of this tree %.1f, smallest of the parent %.1f: %s" % (tree, low, "PASS" if tree >= low else "FAIL"))
    cases = GRAD_CASES if a.gradients else CASES
    med = {case: [] for case in cases}
    rec = {}
    for rnd in range(a.rounds):
        for case in cases:
            o = json.loads(run_child(me + ["--child", case, "--repeats", str(a.repeats)] + (["--layers"] if rnd == 0 else []), env0, 300).strip().splitlines()[-1])
            med[case].append(statistics.median(o["ms_per_step"]))
            print("    case %s: %.4f ms per step" % (case, med[case][-1]), file=sys.stderr, flush=True)
            if "record_ms" in o:
                rec[case] = o["record_ms"]
    say("(b) ms per step (host clock, %d-step blocks, process medians of %d blocks; %d processes per case; 2x: mode 2 with the cross sums, 2x/4: and a stride of 4)"
        % (STEPS, a.repeats, a.rounds))
    for case in cases:
        say("    mode %s: %s; median %.4f (+%.4f over mode 0)" % (case, ", ".join("%.4f" % v for v in med[case]), statistics.median(med[case]),
                                                                statistics.median(med[case]) - statistics.median(med["0"])))
    cells = N ** 3
    if a.gradients:
        tmp = tempfile.mkdtemp(prefix="time_grad_cost_")
        run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me + ["--child", "1g", "--repeats", "1"], env0, 600)
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
        if len(found) != 1:
            raise SystemExit("time_stats_cost: no kernel trace under " + tmp)
        grad, acc = durations(found[0], "k_time_grad<")[WARMUP:], durations(found[0], "k_time_stats_v4<float, 1>")[WARMUP:]
        if len(grad) != STEPS or len(acc) != STEPS:
            raise SystemExit("time_stats_cost: %d gradient and %d mode-1 launches in the trace, %d steps" % (len(grad), len(acc), STEPS))
        say("(e) device time over the same %d steps of one trace (rocprofv3 --kernel-trace, case 1g), median (min - max) us" % STEPS)
        for name, d, nb in (("k_time_stats_v4<float, 1>", acc, BYTES["1"]), ("k_time_grad<float>", grad, GRAD_BYTES)):
            say("    %s: %.1f (%.1f - %.1f); %d B/cell with reads and writes apart: %s"
                % (name, statistics.median(d), min(d), max(d), nb, rate_text(nb * cells, statistics.median(d))))
        say("    the gradient kernel's median %.1f against the mode-1 kernel's %.1f: %s"
            % (statistics.median(grad), statistics.median(acc), "PASS" if statistics.median(grad) <= statistics.median(acc) else "FAIL"))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    say("(c) device time of the kernels (rocprofv3 --kernel-trace), median (min - max) us")
    rate = {}
    for case in ("1", "2", "2x"):
        # fresh processes, `--rounds` per side, the sides alternating and taking turns to go first; the launches of a side are pooled
        acc, lay, pacc, per = [], [], [], {"tree": [], "parent": []}
        for rnd in range(a.rounds):
            sides = ["tree"] + (["parent"] if envp is not None and case != "2x" else [])
            for side in (sides if rnd % 2 else sides[::-1]):
                d, l = traced(me, case, env0 if side == "tree" else envp)
                per[side].append(statistics.median(d))
                if side == "tree":
                    acc += d
                    lay += l
                else:
                    pacc += d
        nb = BYTES[case] * cells
        rate[case] = tbs(nb, statistics.median(acc))
        say("    mode %s accumulation k_time_stats_v4 / _v1: %.1f (%.1f - %.1f) us over %d launches of %d processes (their medians: %s); %d B/cell: %s"
            % (case, statistics.median(acc), min(acc), max(acc), len(acc), len(per["tree"]), ", ".join("%.1f" % v for v in per["tree"]), BYTES[case],
               rate_text(nb, statistics.median(acc))))
        if pacc:
            say("    mode %s accumulation on the parent's library: %.1f (%.1f - %.1f) us over %d launches of %d processes (their medians: %s); this tree's median %.1f against the parent's largest %.1f: %s"
                % (case, statistics.median(pacc), min(pacc), max(pacc), len(pacc), len(per["parent"]), ", ".join("%.1f" % v for v in per["parent"]),
                   statistics.median(acc), max(pacc), "PASS" if statistics.median(acc) <= max(pacc) else "FAIL"))
        say("    mode %s statistic layer k_time_stats_layer: %.1f (%.1f - %.1f) us over %d launches (not tuned)"
            % (case, statistics.median(lay), min(lay), max(lay), len(lay)))
    say("    cross kernel %.2f TB/s against %.1f x the mode 2 kernel's %.2f TB/s = %.2f: %s"
        % (rate["2x"], CROSS_RATE_SHARE, rate["2"], CROSS_RATE_SHARE * rate["2"], "PASS" if rate["2x"] >= CROSS_RATE_SHARE * rate["2"] else "FAIL"))
    for case in rec:
        say("    mode %s record at 54 x 54 x 52 (fs3d_get_layer, returns synchronised), host clock ms per source.moment: %s"
            % (case, "; ".join("%s: %.3f" % (k, statistics.median(v)) for k, v in sorted(rec[case].items()))))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
