"""What one output record costs: fs3d_get_layer of this tree's library against another build's (the parent commit's), fp32, one GPU.

  python tools/get_layer_cost.py --parent-lib DIR/libfs3d_hip.so [--parent-driver DIR/fs3d_run]   -> profiles/get_layer_cost.json

(a) per call.  Two grids, heart_us (96 x 160 x 128; its config samples 48 x 80 x 32) and a 256^3 box with an obstacle (50^3), each
    also at full resolution (0, 0, 0).  Every measurement is a fresh child process that loads ONE library (FS3D_LIB_PATH, as
    tools/ab_env.py runs other builds), makes one time step, warms the call up and takes the host clock around `--repeats` calls
    of fs3d_get_layer, which returns synchronised.  The two libraries alternate, `--rounds` children each; the samples of a
    library are pooled: median (min - max).  The children also hash what the call returned: the two builds must agree.
    The other build does not export fs3d_get_layer_info; this tree's row carries its bytes.
(b) the driver.  fs3d_run ... GPU moving --time-geometry --time-output on heart_us, 12 steps, this tree's driver and the other
    build's alternating after a warm-up pair: the whole step of both (the --time-geometry line) and this tree's split of the
    output (the --time-output line, which the other build does not print).  The _res.nc files of the two must be the same bytes,
    in `moving`, plain single-context and `GPU 2 --same-device` mode.
Every GPU child runs under its own `timeout`; the tool stops at the first child that fails.
"""
import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_ENTRIES = ("fs3d_get_layer_rows", "fs3d_get_layer_dev", "fs3d_get_layer_info")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
DEFAULT_OUT = os.path.join(ROOT, "profiles", "get_layer_cost.json")


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def case_nodes(case):
    """(nodes, params, the config's output dims)"""
    from cmc_fluid_solver_amd import capi, grids
    if case == "heart_us":
        import refgolden as RG
        from cmc_fluid_solver_amd import shape2d
        fx = RG.Fixture("heart_us", "f32")
        cfg = fx.cfg()
        nodes = shape2d.load_shape2d(fx.data_path, cfg.dx, cfg.dy, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT, fx.meta["align"])[0]
        return nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), (cfg.outdimx, cfg.outdimy, cfg.outdimz)
    return grids.box_with_obstacle(256, 256, 256), capi.fluid_params(np.float32, 200.0, 0.72, 1.4), (50, 50, 50)


def child(case, repeats):
    """One library (FS3D_LIB_PATH), one grid: prints one JSON line."""
    from cmc_fluid_solver_amd import capi
    import ctypes as C
    old = not hasattr(C.CDLL(capi.LIB_PATH), NEW_ENTRIES[0])
    if old:                                  # a build from before these entries: they stay unbound in this process
        for name in NEW_ENTRIES:
            capi.SYMBOLS.pop(name)
    nodes, params, cfg_od = case_nodes(case)
    s = capi.Solver(nodes, params, np.float32)
    s.UpdateBoundaries()
    s.TimeStep(np.float32(1e-3), 1, 1, True)
    s.UpdateBoundaries()
    s.TimeStep(np.float32(1e-3), 1, 1, True)                 # `next` now holds the first step's layer
    out = {"case": case, "dims": list(nodes.shape), "library": capi.LIB_PATH, "calls": {}}
    for outdims in (cfg_od, (0, 0, 0)):
        od = [o or d for o, d in zip(outdims, nodes.shape)]
        V, T = np.empty(od + [3], np.float32), np.empty(od, np.float64)
        pV, pT = V.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p)
        for _ in range(3):
            s._chk(s.lib.fs3d_get_layer(s.h, pV, pT, *outdims))
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            st = s.lib.fs3d_get_layer(s.h, pV, pT, *outdims)
            ms.append((time.perf_counter() - t0) * 1e3)
            s._chk(st)
        row = {"ms": ms, "sha256": hashlib.sha256(V.tobytes() + T.tobytes()).hexdigest()}
        if not old:
            row["get_layer_info"] = s.get_layer_info()
        out["calls"]["x".join(str(o) for o in outdims)] = row
    s.close()
    print(json.dumps(out))


def run_child(cmd, env, seconds):
    """A GPU child under its own time limit; the first failure ends the tool."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("get_layer_cost: %s ended with status %d\n%s" % (" ".join(cmd), r.returncode, (r.stdout + r.stderr)[-2000:]))
    return r.stdout


def measure_calls(a, libs):
    res = {}
    for case in ("heart_us", "box256"):
        rows = {name: {} for name in libs}
        for _ in range(a.rounds):
            for name, lib in libs.items():
                env = dict(os.environ)
                if lib:
                    env["FS3D_LIB_PATH"] = lib
                else:
                    env.pop("FS3D_LIB_PATH", None)
                o = json.loads(run_child([sys.executable, os.path.abspath(__file__), "--child", case, "--repeats", str(a.repeats)], env, 600).strip().splitlines()[-1])
                for od, row in o["calls"].items():
                    acc = rows[name].setdefault(od, {"ms": [], "sha256": row["sha256"]})
                    acc["ms"] += row["ms"]
                    if acc["sha256"] != row["sha256"]:
                        raise SystemExit("get_layer_cost: %s %s: two runs of one library differ" % (case, od))
                    if "get_layer_info" in row:
                        acc["get_layer_info"] = row["get_layer_info"]
                dims = o["dims"]
        out = {"dims": dims, "cells": int(np.prod(dims)), "calls": {}}
        for od in rows["this_tree"]:
            t, p = rows["this_tree"][od], rows["parent"][od]
            if t["sha256"] != p["sha256"]:
                raise SystemExit("get_layer_cost: %s %s: the two libraries return different records" % (case, od))
            st, sp = stats(t["ms"]), stats(p["ms"])
            out["calls"][od] = {"this_tree": st, "parent": sp, "same_bytes": True, "get_layer_info": t["get_layer_info"],
                                "ranges_overlap": not (st["max_ms"] < sp["min_ms"] or sp["max_ms"] < st["min_ms"])}
            print("%-9s %-11s this tree %.3f (%.3f - %.3f) ms   parent %.3f (%.3f - %.3f) ms" % (
                case, od, st["median_ms"], st["min_ms"], st["max_ms"], sp["median_ms"], sp["min_ms"], sp["max_ms"]), flush=True)
        res[case] = out
    return res


def measure_driver(a, drivers):
    data, cfgf = (os.path.join(INPUTS, f) for f in ("heart_us_2D_data.txt", "heart_us_2D_config.txt"))
    tmp = tempfile.mkdtemp(prefix="get_layer_cost_")
    res = {"steps": 12, "runs": a.driver_runs}

    def run(name, words, tag):
        prefix = os.path.join(tmp, "%s_%s" % (name, tag))
        o = run_child([drivers[name], data, prefix, cfgf, "align"] + words + ["--steps", "12"], dict(os.environ), 600)
        return o, open(prefix + "_res.nc", "rb").read()

    moving = ["GPU", "moving", "--time-geometry", "--time-output"]
    for name in drivers:
        run(name, moving, "warm")
    step, split, same = {name: [] for name in drivers}, {"GetLayer": [], "AppendLayer": []}, True
    for k in range(a.driver_runs):
        nc = {}
        for name in drivers:
            o, nc[name] = run(name, moving, "m%d" % k)
            step[name].append(float(re.search(r"; step ([0-9.]+)\n", o).group(1)))
            m = re.search(r"Result output per record \(host clock, ms\): GetLayer ([0-9.]+), AppendLayer ([0-9.]+); (\d+) records", o)
            if name == "this_tree":
                split["GetLayer"].append(float(m.group(1))); split["AppendLayer"].append(float(m.group(2))); res["records"] = int(m.group(3))
        same = same and nc["this_tree"] == nc["parent"]
    res["moving"] = {"step_ms": {name: stats(v) for name, v in step.items()}, "this_tree_per_record_ms": {k: stats(v) for k, v in split.items()},
                     "res_nc_same_bytes": same}
    for tag, words in (("single", ["GPU"]), ("gpu2_same_device", ["GPU", "2", "--same-device"])):
        nc = {name: run(name, words, tag)[1] for name in drivers}
        res[tag] = {"res_nc_same_bytes": nc["this_tree"] == nc["parent"], "res_nc_bytes": len(nc["this_tree"])}
    print("driver:", json.dumps(res), flush=True)
    return res


def tree_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="internal: measure this grid with the library of FS3D_LIB_PATH and print one JSON line")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="children per library and grid, the libraries alternating")
    ap.add_argument("--parent-lib", default=None, help="libfs3d_hip.so of the build to compare with (the parent commit's)")
    ap.add_argument("--parent-driver", default=None, help="its fs3d_run; without it the driver rows are left out")
    ap.add_argument("--driver-runs", type=int, default=3)
    ap.add_argument("--commit", default=None, help="what to record as this tree's commit (default: git rev-parse of the tree)")
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    if not a.parent_lib or not os.path.isfile(a.parent_lib):
        raise SystemExit("get_layer_cost: --parent-lib: the library of the build to compare with")
    from cmc_fluid_solver_amd import build as B
    res = {"commit": a.commit or tree_commit(), "parent_commit": a.parent_commit, "precision": "fp32", "repeats": a.repeats, "rounds": a.rounds,
           "note": "host clock around fs3d_get_layer (returns synchronised), 3 warm-up calls, the two libraries in alternating fresh processes, samples "
                   "pooled per library: median (min - max); get_layer_info: samples, bytes device-to-host, device allocations of this tree's call"}
    res["per_call"] = measure_calls(a, {"this_tree": None, "parent": os.path.abspath(a.parent_lib)})
    if a.parent_driver:
        res["driver_heart_us"] = measure_driver(a, {"this_tree": B.DRIVER, "parent": os.path.abspath(a.parent_driver)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
