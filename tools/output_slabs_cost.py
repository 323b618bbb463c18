"""What a filtered or derived result record costs on x-slabs (FS3D_OPT_OUTPUT_SLABS; k_get_layer_box, k_get_layer_finish,
k_type_planes), fp32, in-process slabs of ONE device, beside the whole-grid record of the same library in the same session.

  python tools/output_slabs_cost.py [--repeats N] [--out FILE]        -> profiles/output_slabs_cost.txt

A 256^3 box with an obstacle -> 54 x 54 x 52 samples.  One child per layout -- the whole grid, 2 slabs, 4 slabs: the same box
kernel, told apart by the child's layout (a library from before the two box kernels became one gives the slabs' kernel a longer
name that begins alike; it is counted as the box kernel too, so FS3D_LIB_PATH may select such a library) -- makes, for the box
mean and for the box-mean vorticity, 3 warm-up records and `--repeats` timed ones: the host clock around the
call on rank 0 (the call returns synchronised; on slabs it holds the exchange, the all-reduce and the waits for the peers).  A second
child of the same layout runs under `rocprofv3 --kernel-trace` (alone): per kernel name the median device duration and the
launches per record; a record's device time is the sum over the names of median x launches per record, over all ranks.  The slabs
of one device run their kernels side by side, and each then lasts as long as all of them together: beside the sum stands the time
the device is busy with the kernels behind the stamps, the union of their intervals per record (a mean over all records).
Expectation, stated before the run and checked here: the slab kernels' summed device time stays within the whole-grid kernel's
plus the whole-grid stamp (k_clear_type) plus the time two planes of the four fields take to copy at the rate the stamp reaches.
The all-reduce moves at most (nranks - 1) * ody * odz * 40 bytes.  Slabs on several devices and RCCL ranks are not measured here.
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

DEFAULT_OUT = os.path.join(ROOT, "profiles", "output_slabs_cost.txt")
DIMS, OUTDIMS = (256, 256, 256), (54, 54, 52)
MODES = (("box mean", 1, 0), ("box-mean vorticity", 1, 1))
LAYOUTS = (1, 2, 4)
WARMUP = 3
KERNELS = ("k_clear_type", "k_type_planes", "k_get_layer_box", "k_get_layer_finish")


def run_child(cmd, seconds):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("output_slabs_cost: %s ended with status %d\n%s" % (" ".join(cmd), r.returncode, (r.stdout + r.stderr)[-2000:]))
    return r.stdout


def child(nslabs, repeats):
    """One layout, every mode; prints one JSON line"""
    from cmc_fluid_solver_amd import capi, grids
    nodes = grids.box_with_obstacle(*DIMS)
    params = capi.fluid_params(np.float32, 200.0, 0.72, 1.4)
    V, T = np.empty(OUTDIMS + (3,), np.float32), np.empty(OUTDIMS, np.float64)

    def work(rank, s):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(1e-3), 1, 1, True)               # `next` holds a step's layer
        s.set_option(capi.OPT_OUTPUT_SLABS, 1)
        res = {}
        for name, filter, vector in MODES:
            s.set_option(capi.OPT_OUTPUT_FILTER, filter)
            s.set_option(capi.OPT_OUTPUT_VECTOR, vector)
            ms = []
            for k in range(WARMUP + repeats):
                t0 = time.perf_counter()
                s.GetLayerRows(V, T, OUTDIMS)
                if k >= WARMUP:
                    ms.append((time.perf_counter() - t0) * 1e3)
            res[name] = ms
        return res
    if nslabs == 1:
        s = capi.Solver(nodes, params, np.float32)
        res = work(0, s)
        s.close()
    else:
        grp = capi.LocalGroup(nodes, params, nslabs, np.float32)
        res = grp.run(work)[0]
        grp.close()
    print(json.dumps({"nslabs": nslabs, "calls_per_mode": WARMUP + repeats, "host_ms": res}))


def kernel_times(path, calls_per_mode):
    """{mode: {kernel: (median us, launches per record)}} from a kernel trace: the records of a mode are consecutive"""
    rows = [r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))

    def name_of(r):
        return [k for k in KERNELS if k in r["Kernel_Name"]][0]
    # the stamp opens every rank's record: split the trace into the modes by the share of stamps seen
    stamps = [k for k, r in enumerate(rows) if name_of(r) == "k_clear_type"]
    per_mode = len(stamps) // len(MODES)
    out = {}
    for m, (mode, _, _) in enumerate(MODES):
        lo = stamps[m * per_mode]
        hi = stamps[(m + 1) * per_mode] if m + 1 < len(MODES) else len(rows)
        by = {}
        for r in rows[lo:hi]:
            by.setdefault(name_of(r), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        out[mode] = {k: (statistics.median(v), len(v) / calls_per_mode) for k, v in by.items()}
        # the slabs of one device run their kernels side by side: the time the device is busy with them is the union of the intervals
        iv = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows[lo:hi] if name_of(r) != "k_clear_type")
        busy, end = 0, 0
        for a, b in iv:
            if b > end:
                busy += b - max(a, end)
                end = b
        out[mode]["busy"] = (busy / 1e3 / calls_per_mode, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", type=int, default=0, help="internal: measure this layout and print one JSON line")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.repeats)
    me = [sys.executable, os.path.abspath(__file__)]
    lines = ["filtered and derived records on x-slabs: 256^3 box with an obstacle -> 54 x 54 x 52, fp32, in-process slabs of one MI355X",
             "host clock per record on rank 0, ms: median (min - max) of %d calls after %d warm-up calls; device time per kernel from a" % (a.repeats, WARMUP),
             "rocprofv3 --kernel-trace run of the same child: median us x launches per record (all ranks)", ""]
    dev = {}
    for nslabs in LAYOUTS:
        o = json.loads(run_child(me + ["--child", str(nslabs), "--repeats", str(a.repeats)], 600).strip().splitlines()[-1])
        tmp = tempfile.mkdtemp(prefix="output_slabs_cost_")
        run_child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] + me + ["--child", str(nslabs), "--repeats", str(a.repeats)], 900)
        found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
        if len(found) != 1:
            raise SystemExit("output_slabs_cost: no kernel trace under " + tmp)
        kt = kernel_times(found[0], o["calls_per_mode"])
        for mode, _, _ in MODES:
            ms = o["host_ms"][mode]
            busy = kt[mode].pop("busy")[0]
            parts = ", ".join("%s %.1f us x %.2g" % (k, v[0], v[1]) for k, v in sorted(kt[mode].items()))
            total = sum(v[0] * v[1] for k, v in kt[mode].items() if k != "k_clear_type")
            dev[nslabs, mode] = (total, kt[mode], busy)
            lines.append("%-11s %-19s host %.3f (%.3f - %.3f) ms; kernels behind the stamp %.1f us per record summed, device busy with them %.1f us per record (mean); %s" % (
                "whole grid" if nslabs == 1 else "%d slabs" % nslabs, mode, statistics.median(ms), min(ms), max(ms), total, busy, parts))
            print(lines[-1], flush=True)
    lines.append("")
    plane_bytes = 2 * 4 * DIMS[1] * DIMS[2] * 4                  # two planes of four fp32 fields
    for mode, _, _ in MODES:
        whole, kt, _ = dev[1, mode]
        stamp_us = kt["k_clear_type"][0]
        stamp_rate = (2 * DIMS[0] * DIMS[1] * DIMS[2]) / (stamp_us * 1e-6)        # bytes of code the stamp streams per second (a floor)
        allow = whole + stamp_us + plane_bytes / stamp_rate * 1e6
        for nslabs in LAYOUTS[1:]:
            got = dev[nslabs, mode][0]
            busy = dev[nslabs, mode][2]
            lines.append("%-19s %d slabs: kernels summed %.1f us against %.1f us (whole-grid kernel %.1f + stamp %.1f + two plane copies %.1f): %s; "
                         "device busy %.1f us: %s; all-reduce at most %d bytes" % (
                             mode, nslabs, got, allow, whole, stamp_us, plane_bytes / stamp_rate * 1e6, "WITHIN" if got <= allow else "ABOVE",
                             busy, "WITHIN" if busy <= allow else "ABOVE", (nslabs - 1) * OUTDIMS[1] * OUTDIMS[2] * 40))
            print(lines[-1], flush=True)
    lines += ["", "Not measured: slabs on several devices, RCCL ranks (compiled, never run)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
