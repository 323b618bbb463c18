"""What fs3d_update_nodes_slab costs per slab, beside fs3d_update_nodes on the whole grid.

    python tools/slab_geometry_cost.py [--ranks 4] [--repeats 10] [--out profiles/slab_geometry_cost.json]

The 256^3 masked case of tools/geometry_update_cost.py (the non_uniform256 nodes and the same with a solid block added, alternating),
fp32.  One whole-grid context takes fs3d_update_nodes; `--ranks` lone slab contexts on the same card (the call talks to no other
rank, so no group is needed) take fs3d_update_nodes_slab one after the other.  Per context: the host clock around the call, copies
included, and the device time alone (fs3d_last_update_device_ms).  Every rank reads the three byte arrays of the GLOBAL grid for
its X lines, so that pass does not shrink with the number of ranks; everything else works on the slab's planes.
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cmc_fluid_solver_amd import capi  # noqa: E402
from cmc_fluid_solver_amd.slab import slab_range  # noqa: E402
from geometry_update_cost import stats, with_block  # noqa: E402


def measure(s, update, geoms, repeats):
    for k in (1, 0, 1, 0):                                  # warm-up: first launches, the buffers the first updates allocate
        update(geoms[k])
    s.enable_timing(True)
    host, dev = [], []
    for r in range(repeats):
        t0 = time.perf_counter(); update(geoms[(r + 1) % 2]); s.synchronize()
        host.append((time.perf_counter() - t0) * 1e3); dev.append(s.last_update_device_ms())
    s.enable_timing(False)
    return {"host_clock": stats(host), "device_time": stats(dev), "allocs_and_frees": s.geometry_info()["device_allocs_and_frees"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab_geometry_cost.json"))
    a = ap.parse_args()
    import refgolden as RG
    fx = RG.Fixture("heart_us", "f32")
    cfg = fx.cfg()
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    ga = RG.Fixture("non_uniform256", "f32").nodes()
    geoms = [ga, with_block(ga)]
    res = {"dims": list(ga.shape), "ranks": a.ranks, "repeats": a.repeats, "precision": "fp32",
           "note": "host clock around calls that end synchronised, copies included; device time from HIP events inside the library"}
    s = capi.Solver(ga, params, np.float32)
    res["single_context_update_nodes"] = measure(s, s.update_nodes, geoms, a.repeats)
    res["single_context_update_nodes_slab"] = measure(s, s.update_nodes_slab, geoms, a.repeats)
    s.close()
    for r in range(a.ranks):
        xr = slab_range(ga.dimx, r, a.ranks)
        s = capi.Solver(ga, params, np.float32, x_range=xr)
        res["slab_%d_planes_%d_%d" % (r, xr[0], xr[1])] = measure(s, s.update_nodes_slab, geoms, a.repeats)
        s.close()
    for k, v in res.items():
        print(k, json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
