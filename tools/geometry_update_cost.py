"""What a change of geometry costs per call, and whether a time step runs as fast on updated tables as on uploaded ones.

    python tools/geometry_update_cost.py [--repeats 20] [--out profiles/geometry_update_cost.json]

Two cases: the heart_us grid (96 x 160 x 128, two geometries of its cycle) and the 256^3 masked case (the non_uniform256 nodes and
the same with a solid block added).  Per case, alternating the two geometries after a warm-up:
  (a) fs3d_upload_nodes per call       -- host clock around the call (it ends synchronised): the only way before fs3d_update_nodes
  (b) fs3d_update_nodes per call       -- host arrays, copies included; host clock
  (c) fs3d_update_nodes_dev per call   -- device arrays; host clock, and the device time alone (HIP events inside the library)
  (d) time per step (G 4, L 2, AUTO, fp32) after an upload and after an update of the same geometry, interleaved, with the spread
Needs the GPU: there is no fallback.  One process, one context per case.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cmc_fluid_solver_amd import capi, grids  # noqa: E402


def with_block(nodes):
    """The same geometry with a solid block (no-slip surface, NODE_OUT inside) set into the fluid around the centre of the NODE_IN cells."""
    g = grids.Nodes(nodes.dimx, nodes.dimy, nodes.dimz, nodes.dx, nodes.dy, nodes.dz,
                    *[np.array(a, copy=True) for a in (nodes.type, nodes.bc_vel, nodes.bc_temp, nodes.vx, nodes.vy, nodes.vz, nodes.T)])
    c = np.argwhere(g.type == grids.NODE_IN).mean(axis=0).astype(int)
    h = [max(3, d // 12) for d in g.shape]
    lo = [max(2, int(c[a]) - h[a]) for a in range(3)]
    hi = [min(g.shape[a] - 3, int(c[a]) + h[a]) for a in range(3)]
    blk = np.zeros(g.shape, bool); blk[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    inner = np.zeros(g.shape, bool); inner[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = True
    fluid = g.type == grids.NODE_IN
    shell = blk & ~inner & fluid
    g.type[shell] = grids.NODE_BOUND; g.bc_vel[shell] = grids.BC_NOSLIP; g.bc_temp[shell] = grids.BC_NOSLIP
    g.vx[shell] = 0; g.vy[shell] = 0; g.vz[shell] = 0
    g.type[inner & fluid] = grids.NODE_OUT
    return g


def arrays(nodes, dtype):
    return [np.ascontiguousarray(nodes.type, np.uint8), np.ascontiguousarray(nodes.bc_vel, np.uint8), np.ascontiguousarray(nodes.bc_temp, np.uint8)] + \
           [np.ascontiguousarray(v, dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def measure(name, ga, gb, params, repeats, steps_per_sample=10):
    import torch
    dtype = np.float32
    s = capi.Solver(ga, params, dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_AUTO)
    host = [arrays(ga, dtype), arrays(gb, dtype)]
    dev = [[torch.from_numpy(a).cuda() for a in h] for h in host]
    torch.cuda.synchronize()
    nseg = (C.c_int * 3)()

    def upload(k):
        s._chk(s.lib.fs3d_upload_nodes(s.h, *[capi._p(a) for a in host[k]], nseg))

    def update(k):
        s._chk(s.lib.fs3d_update_nodes(s.h, *[capi._p(a) for a in host[k]], nseg))

    def update_dev(k):
        s._chk(s.lib.fs3d_update_nodes_dev(s.h, *[C.c_void_p(t.data_ptr()) for t in dev[k]], nseg))

    def clock(fn, k):
        t0 = time.perf_counter(); fn(k); s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def step_ms():
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps_per_sample):
            s.time_step_async(dtype(0.01), 4, 2)
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps_per_sample

    out = {"dims": list(ga.shape), "cells": ga.ncells}
    for fn in (upload, update, update_dev):                 # warm-up: first launches, the buffers the first update allocates
        for k in (1, 0):
            fn(k)
    out["upload_nodes"] = stats([clock(upload, (r + 1) % 2) for r in range(repeats)])
    update(0)
    out["update_nodes"] = stats([clock(update, (r + 1) % 2) for r in range(repeats)])
    s.enable_timing(True)
    host_ms, dev_ms = [], []
    for r in range(repeats):
        host_ms.append(clock(update_dev, (r + 1) % 2)); dev_ms.append(s.last_update_device_ms())
    s.enable_timing(False)
    out["update_nodes_dev"] = stats(host_ms)
    out["update_nodes_dev_device_time"] = stats(dev_ms)
    # the same geometry (B) through both paths, interleaved; layers restarted from its nodes each time so that both time the same state
    info = {}
    t_up, t_ud = [], []
    step_ms()
    for r in range(repeats):
        for path, fn, acc in (("upload", upload, t_up), ("update", update_dev, t_ud)):
            fn(1)
            s._chk(s.lib.fs3d_init_layers_from_nodes(s.h))
            info[path] = s.geometry_info()
            acc.append(step_ms())
    out["step_after_upload"], out["step_after_update"] = stats(t_up), stats(t_ud)
    out["sweep_kernels"] = s.last_sweep_kernels()
    out["tables_equal"] = all(info["upload"][k] == info["update"][k] for k in capi.Solver.GEOMETRY_INFO[:13])
    out["geometry_info"] = info["update"]
    out["ratio_update_over_upload"] = out["update_nodes"]["median_ms"] / out["upload_nodes"]["median_ms"]
    out["update_dev_device_time_over_step"] = out["update_nodes_dev_device_time"]["median_ms"] / out["step_after_update"]["median_ms"]
    s.close()
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse of the tree)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_update_cost.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    torch.cuda.init()                       # torch opens the device before the library does (its tensors are handed to the library)
    import refgolden as RG
    from cmc_fluid_solver_amd import shape2d
    commit = a.commit
    try:
        commit = commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    res = {"device": torch.cuda.get_device_name(0), "commit": commit, "repeats": a.repeats, "precision": "fp32",
           "note": "host clock around calls that end synchronised; device time from HIP events inside the library; step = G 4, L 2, AUTO"}
    fx = RG.Fixture("heart_us", "f32")
    cfg = fx.cfg()
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    h = [shape2d.load_shape2d(fx.data_path, cfg.dx, cfg.dy, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT, fx.meta["align"], time=t)[0]
         for t in (fx.meta["grid_times"][0], fx.meta["grid_times"][3])]
    res["heart_us"] = measure("heart_us", h[0], h[1], params, a.repeats)
    n256 = RG.Fixture("non_uniform256", "f32").nodes()
    res["non_uniform256"] = measure("non_uniform256", n256, with_block(n256), params, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
