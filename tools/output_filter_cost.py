"""What the filtered and derived result records cost (FS3D_OPT_OUTPUT_FILTER, FS3D_OPT_OUTPUT_VECTOR, FS3D_OPT_OUTPUT_GRADIENT; k_get_layer_box), fp32, one GPU.

  python tools/output_filter_cost.py --parent-lib DIR/libfs3d_hip.so [--out FILE]        -> profiles/output_filter_cost.json

(a) the default record is not slower.  fs3d_get_layer with both options 0, heart_us (96 x 160 x 128 -> 48 x 80 x 32) and a 256^3 box with
    an obstacle (-> 50^3): the children of tools/get_layer_cost.py (one library per fresh process, FS3D_LIB_PATH; host clock around
    `--repeats` calls, which return synchronised), `--rounds` rounds with the parent's library first in every round, then as many with
    this tree's first.  Verdict per shape, the rule of profiles/voxel_rule_shared_cost.txt, set before the run: the median of this
    tree's process medians is no larger than the largest of the parent's process medians.  The records of the two must be the same bytes.
(b) what a filtered record costs.  One child of this tree's library per grid makes, mode after mode -- default, box mean, point
    vorticity, box-mean vorticity, point invariants, box-mean invariants (FS3D_OPT_OUTPUT_GRADIENT 1) -- 3 warm-up calls and `--repeats` timed ones (host clock).  A second child does the same under
    `rocprofv3 --kernel-trace` (alone: no counters, no other tracing): the device duration of every k_clear_type and of the kernel
    behind it on the stream, call by call, from the trace's timestamps.  Each kernel is set beside the bytes its shape says it
    moves -- k_get_layer_box: 18 B per source cell (2 B of code and four reals) plus 20 B per sample; k_clear_type: the 2 B of code
    per cell (the same table) plus 16 B per NODE_OUT cell -- as a rate and as a share of the 8 TB/s peak and of the 5.3 - 5.8 TB/s a
    copy reaches.  The invariants read 18 neighbour values where the curl reads 12, behind the same seven codes:
    the expectation, stated before the run, is that the box-mean invariants' kernel stays within 1.5 x the box-mean vorticity's of
    the same session (reported as invariants_over_vorticity; no threshold beyond that: a record is taken per output record).
    `--skip-default --cases box256` runs (b) alone on the 256^3 box.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEFAULT_OUT = os.path.join(ROOT, "profiles", "output_filter_cost.json")
GET_LAYER_COST = os.path.join(ROOT, "tools", "get_layer_cost.py")
# (name, FS3D_OPT_OUTPUT_FILTER, FS3D_OPT_OUTPUT_VECTOR, FS3D_OPT_OUTPUT_GRADIENT)
MODES = (("default", 0, 0, 0), ("box mean", 1, 0, 0), ("point vorticity", 0, 1, 0), ("box-mean vorticity", 1, 1, 0), ("point invariants", 0, 0, 1),
         ("box-mean invariants", 1, 0, 1))
INVARIANTS_EXPECTED = 1.5
CASES = ("box256", "heart_us")
WARMUP = 3
PEAK_TBS, COPY_TBS = 8.0, (5.3, 5.8)


def stats(v, unit):
    return {"median_" + unit: statistics.median(v), "min_" + unit: min(v), "max_" + unit: max(v), "n": len(v)}


def run_child(cmd, env, seconds):
    """A GPU child under its own time limit; the first failure ends the tool."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("output_filter_cost: %s ended with status %d\n%s" % (" ".join(cmd), r.returncode, (r.stdout + r.stderr)[-2000:]))
    return r.stdout


def child(case, repeats):
    """This tree's library, one grid: every mode at the config's output dims; prints one JSON line."""
    import ctypes as C
    from cmc_fluid_solver_amd import capi, grids
    from get_layer_cost import case_nodes
    nodes, params, od = case_nodes(case)
    s = capi.Solver(nodes, params, np.float32)
    for _ in range(2):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(1e-3), 1, 1, True)             # `next` holds a step's layer
    V, T = np.empty(list(od) + [3], np.float32), np.empty(list(od), np.float64)
    pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
    out = {"case": case, "dims": list(nodes.shape), "outdims": list(od), "cells": int(nodes.ncells), "out_cells": nodes.count(grids.NODE_OUT),
           "fluid_cells": nodes.count(grids.NODE_IN), "samples": int(np.prod(od)), "modes": {}}
    for name, filter, vector, gradient in MODES:
        s.set_option(capi.OPT_OUTPUT_FILTER, filter)
        s.set_option(capi.OPT_OUTPUT_VECTOR, vector)
        s.set_option(capi.OPT_OUTPUT_GRADIENT, gradient)
        ms = []
        for k in range(WARMUP + repeats):
            t0 = time.perf_counter()
            st = s.lib.fs3d_get_layer(s.h, pV, pT, *od)
            if k >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
            s._chk(st)
        out["modes"][name] = {"host_ms": ms, "calls": WARMUP + repeats}
    s.close()
    print(json.dumps(out))


def default_record(a, libs):
    """(a): the children of get_layer_cost.py, alternating; per shape the process medians and the verdict"""
    res = {}
    for case in CASES:
        med, sha = {name: [] for name in libs}, set()
        for order in (("parent", "this_tree"), ("this_tree", "parent")):
            for _ in range(a.rounds):
                for name in order:
                    env = dict(os.environ)
                    env.pop("FS3D_LIB_PATH", None)
                    if libs[name]:
                        env["FS3D_LIB_PATH"] = libs[name]
                    o = json.loads(run_child([sys.executable, GET_LAYER_COST, "--child", case, "--repeats", str(a.repeats)], env, 300).strip().splitlines()[-1])
                    key = [k for k in o["calls"] if k != "0x0x0"][0]
                    med[name].append({"order": order[0] + " first", "median_ms": statistics.median(o["calls"][key]["ms"]), "min_ms": min(o["calls"][key]["ms"]),
                                      "max_ms": max(o["calls"][key]["ms"])})
                    sha.add(o["calls"][key]["sha256"])
        tree = statistics.median(m["median_ms"] for m in med["this_tree"])
        worst = max(m["median_ms"] for m in med["parent"])
        res[case] = {"outdims": key, "processes": med, "same_bytes": len(sha) == 1, "this_tree_median_of_process_medians_ms": tree,
                     "parent_median_of_process_medians_ms": statistics.median(m["median_ms"] for m in med["parent"]),
                     "parent_largest_process_median_ms": worst, "pass": bool(tree <= worst and len(sha) == 1)}
        print("(a) %-9s %s: this tree %.4f ms, parent's largest %.4f ms, same bytes %s: %s" % (case, key, tree, worst, len(sha) == 1,
                                                                                            "PASS" if res[case]["pass"] else "FAIL"), flush=True)
    return res


def kernel_pairs(path):
    """(k_clear_type us, the kernel behind it us, its name) per fs3d_get_layer call of a kernel trace, in launch order"""
    rows = [r for r in csv.DictReader(open(path)) if "k_clear_type" in r["Kernel_Name"] or "k_get_layer" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    pairs = []
    for k in range(0, len(rows) - 1, 2):
        if "k_clear_type" not in rows[k]["Kernel_Name"] or "k_get_layer" not in rows[k + 1]["Kernel_Name"]:
            raise SystemExit("output_filter_cost: the trace does not alternate k_clear_type and a k_get_layer kernel at row %d" % k)
        pairs.append((us[k], us[k + 1], "k_get_layer_box" if "k_get_layer_box" in rows[k + 1]["Kernel_Name"] else "k_get_layer"))
    return pairs


def rate(nbytes, us):
    tbs = nbytes / (us * 1e-6) / 1e12
    return {"bytes": int(nbytes), "TB_per_s": tbs, "share_of_peak": tbs / PEAK_TBS, "share_of_copy_rate": [tbs / COPY_TBS[1], tbs / COPY_TBS[0]]}


def filtered_record(a):
    res = {}
    env = dict(os.environ)
    env.pop("FS3D_LIB_PATH", None)
    me = [sys.executable, os.path.abspath(__file__)]
    for case in a.cases:
        o = json.loads(run_child(me + ["--child", case, "--repeats", str(a.repeats)], env, 300).strip().splitlines()[-1])
        tmp = tempfile.mkdtemp(prefix="output_filter_cost_")
        run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me + ["--child", case, "--repeats", str(a.repeats)], env, 600)
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
        if len(found) != 1:
            raise SystemExit("output_filter_cost: no kernel trace under " + tmp)
        pairs = kernel_pairs(found[0])
        calls = sum(m["calls"] for m in o["modes"].values())
        if len(pairs) != calls:
            raise SystemExit("output_filter_cost: %d calls, %d kernel pairs in the trace" % (calls, len(pairs)))
        at = 0
        for name, filter, vector, gradient in MODES:
            m = o["modes"][name]
            mine = pairs[at + WARMUP:at + m["calls"]]
            at += m["calls"]
            kernel = "k_get_layer_box" if filter or vector or gradient else "k_get_layer"
            assert all(p[2] == kernel for p in mine), (name, kernel)
            clear, layer = stats([p[0] for p in mine], "us"), stats([p[1] for p in mine], "us")
            row = {"host_clock_per_call": stats(m.pop("host_ms"), "ms"), "kernel": kernel, "kernel_device": layer, "k_clear_type_device": clear,
                   "kernel_over_k_clear_type": layer["median_us"] / clear["median_us"],
                   "k_clear_type_rate": rate(2 * o["cells"] + 16 * o["out_cells"], clear["median_us"])}
            if filter:                                     # (the point modes read one cell per sample and the curl's neighbours: latency, not a byte stream)
                row["kernel_rate"] = rate(18 * o["cells"] + 20 * o["samples"], layer["median_us"])
            m.update(row)
            print("(b) %-9s %-19s host %.3f ms; %s %.1f (%.1f - %.1f) us; k_clear_type %.1f (%.1f - %.1f) us" % (
                case, name, m["host_clock_per_call"]["median_ms"], kernel, layer["median_us"], layer["min_us"], layer["max_us"],
                clear["median_us"], clear["min_us"], clear["max_us"]), flush=True)
        ratio = o["modes"]["box-mean invariants"]["kernel_device"]["median_us"] / o["modes"]["box-mean vorticity"]["kernel_device"]["median_us"]
        o["invariants_over_vorticity"] = {"box_mean_kernels": ratio, "expected_at_most": INVARIANTS_EXPECTED, "as_expected": bool(ratio <= INVARIANTS_EXPECTED)}
        print("(b) %-9s box-mean invariants / box-mean vorticity = %.2f (expected: at most %.1f)" % (case, ratio, INVARIANTS_EXPECTED), flush=True)
        res[case] = o
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="internal: measure this grid with this tree's library and print one JSON line")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="(a): children per library and order")
    ap.add_argument("--parent-lib", default=None, help="libfs3d_hip.so of the parent commit's build")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--skip-default", action="store_true", help="leave out (a)")
    ap.add_argument("--cases", nargs="+", default=list(CASES), choices=CASES, help="(b): the grids")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    if not a.skip_default and (not a.parent_lib or not os.path.isfile(a.parent_lib)):
        raise SystemExit("output_filter_cost: --parent-lib: the library of the build to compare with (or --skip-default)")
    res = {"commit": a.commit, "parent_commit": a.parent_commit, "precision": "fp32", "repeats": a.repeats, "rounds": a.rounds,
           "note": "(a) host clock around fs3d_get_layer with both options 0, fresh processes alternating, parent first then this tree first; "
                   "(b) host clock per call, and device durations of the two kernels of a call from a rocprofv3 --kernel-trace run of the same child"}
    if not a.skip_default:
        res["default_record"] = default_record(a, {"this_tree": None, "parent": os.path.abspath(a.parent_lib)})
    res["filtered_record"] = filtered_record(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
