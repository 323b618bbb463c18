"""Parent against this tree, for a change of the result-record path that must change no speed: fresh processes alternating the two
libraries (FS3D_LIB_PATH), `--rounds` rounds with the parent's first, then as many with this tree's first, in one session -- the
process that runs second reads higher whichever library it loads.

  python tools/output_records_ab.py --parent-lib DIR/libfs3d_hip.so [--what a,b,c] [--side NAME=LIB ...] [--out FILE]
                                                                                      -> profiles/output_records_one_body.json
(a) the whole-grid record: the children of tools/output_filter_cost.py, 256^3 box with an obstacle -> 50^3 -- box mean, point
    vorticity, box-mean vorticity; per process the median host clock around the call, and from a second process under
    `rocprofv3 --kernel-trace` (alone) the median device time of the kernel behind the stamp.
(b) the slab records: the children of tools/output_slabs_cost.py on 2 and 4 in-process slabs -- box mean and box-mean vorticity; per
    process the median host clock per record on rank 0, and from a traced process the summed device time of the kernels behind the
    stamp (median x launches per record, all ranks).
(c) the default path: python bench.py --gpus 1 --steps 20 --warmup 5, Mcells/s.
Verdict per metric, DESIGN section 7, set before the run: (a), (b) the median of this tree's process medians is no larger than the
largest of the parent's; (c) this tree's median is no lower than the parent's smallest.  A further `--side` is measured in the
same alternation and judged by the same rule.  Every GPU child runs under its own `timeout`; the tool stops at the first that fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import output_filter_cost as FC  # noqa: E402
import output_slabs_cost as SC  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "output_records_one_body.json")


def run(cmd, lib, seconds, trace=False):
    """One GPU child with the library `lib` (None: this tree's); with `trace` under rocprofv3 --kernel-trace: (stdout, trace csv)"""
    env = dict(os.environ)
    env.pop("FS3D_LIB_PATH", None)
    if lib:
        env["FS3D_LIB_PATH"] = lib
    tmp = tempfile.mkdtemp(prefix="output_records_ab_")
    full = (["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--"] if trace else []) + cmd
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + full, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("output_records_ab: %s ended with status %d\n%s" % (" ".join(full), r.returncode, (r.stdout + r.stderr)[-2000:]))
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp) for f in fs if f.endswith("kernel_trace.csv")]
    if trace and len(found) != 1:
        raise SystemExit("output_records_ab: no kernel trace under " + tmp)
    return r.stdout, (found[0] if trace else None)


def whole_grid(lib, repeats):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "output_filter_cost.py"), "--child", "box256", "--repeats", str(repeats)]
    o = json.loads(run(cmd, lib, 300)[0].strip().splitlines()[-1])
    pairs = FC.kernel_pairs(run(cmd, lib, 600, trace=True)[1])
    out, at = {}, 0
    for name, _, _ in FC.MODES:
        calls = o["modes"][name]["calls"]
        if name != "default":
            out["whole grid, %s, host ms" % name] = statistics.median(o["modes"][name]["host_ms"])
            out["whole grid, %s, kernel us" % name] = statistics.median(p[1] for p in pairs[at + FC.WARMUP:at + calls])
        at += calls
    assert at == len(pairs)
    return out


def slabs(lib, repeats):
    out = {}
    for nslabs in (2, 4):
        cmd = [sys.executable, os.path.join(ROOT, "tools", "output_slabs_cost.py"), "--child", str(nslabs), "--repeats", str(repeats)]
        o = json.loads(run(cmd, lib, 600)[0].strip().splitlines()[-1])
        kt = SC.kernel_times(run(cmd, lib, 900, trace=True)[1], o["calls_per_mode"])
        for mode, _, _ in SC.MODES:
            out["%d slabs, %s, host ms" % (nslabs, mode)] = statistics.median(o["host_ms"][mode])
            out["%d slabs, %s, kernels summed us" % (nslabs, mode)] = sum(v[0] * v[1] for k, v in kt[mode].items() if k not in ("k_clear_type", "busy"))
    return out


def bench(lib, repeats):
    o = run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, 600)[0]
    return {"bench.py, Mcells/s": json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1])["value"]}


PARTS = {"a": whole_grid, "b": slabs, "c": bench}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libfs3d_hip.so of the parent commit's build")
    ap.add_argument("--side", action="append", default=[], metavar="NAME=LIB", help="a further library, measured in the same alternation")
    ap.add_argument("--what", default="a,b,c")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="processes per library and order")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent-commit", default=None)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    libs = {"parent": os.path.abspath(a.parent_lib), "this_tree": None}
    libs.update({s.split("=", 1)[0]: os.path.abspath(s.split("=", 1)[1]) for s in a.side})
    for lib in libs.values():
        if lib and not os.path.isfile(lib):
            raise SystemExit("output_records_ab: no library " + lib)
    others = [n for n in libs if n != "parent"]
    res = {"commit": a.commit, "parent_commit": a.parent_commit, "precision": "fp32", "repeats": a.repeats, "rounds": a.rounds,
           "rule": "per metric: the median of a side's process values against the parent's largest (Mcells/s: smallest); "
                   "fresh processes alternating, the parent first in the first half of the rounds, last in the second", "metrics": {}}
    for part in a.what.split(","):
        per = {n: [] for n in libs}
        for first in (True, False):
            order = ["parent"] + others if first else others + ["parent"]
            for _ in range(a.rounds):
                for n in order:
                    t0 = time.time()
                    per[n].append(PARTS[part](libs[n], a.repeats))
                    print("(%s) %-10s %3.0f s %s" % (part, n, time.time() - t0, json.dumps(per[n][-1])), flush=True)
        for metric in per["parent"][0]:
            up = metric.endswith("Mcells/s")
            vals = {n: [p[metric] for p in per[n]] for n in libs}
            bound = min(vals["parent"]) if up else max(vals["parent"])
            row = {"parent": vals["parent"], "parent_median": statistics.median(vals["parent"]), "parent_bound": bound}
            for n in others:
                med = statistics.median(vals[n])
                row[n] = vals[n]
                row[n + "_median"] = med
                row[n + "_pass"] = bool(med >= bound if up else med <= bound)
                print("%-45s %-10s median %.4f, parent median %.4f, parent's %s %.4f: %s" % (
                    metric, n, med, row["parent_median"], "smallest" if up else "largest", bound, "PASS" if row[n + "_pass"] else "FAIL"), flush=True)
            res["metrics"][metric] = row
        with open(a.out, "w") as f:                            # after every part: what was measured survives a later failure
            json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
