"""What fs3d_fill_fresh_cells costs beside the geometry update it follows.

    python tools/fresh_cells_cost.py [--sizes 128 256] [--steps 20] [--warmup 3] [--out profiles/fresh_cells_cost.txt]

The translating sphere of tests/wall_velocity_cases.py (20 faces, walls at the mesh's velocity and temperature 0, conservative
voxelisation) scaled from its 28 x 35 x 28 grid to N^3, fp32, FS3D_OPT_FRESH_CELLS on.  Per step: fs3d_update_nodes_shape3d_vel of
the moved mesh, then fs3d_fill_fresh_cells on FS3D_LAYER_CUR -- no time step in between: the fill's cost depends on the types, not
on the values.  Two motions per size: half a cell per step, as in the test, and the test's motion scaled with the grid (N / 56
cells per step: a thicker shell, several rounds).  Printed per step: the update's device time (fs3d_last_update_device_ms), the
fill's (fs3d_last_fill_device_ms: the snapshot's copy kernel, the classifying pass and the rounds), the host clock around the fill
call, and the fill's counts.  Device times come from HIP events inside the library, with fs3d_enable_timing on.
Needs the GPU: there is no fallback."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cmc_fluid_solver_amd import capi, grids  # noqa: E402

PARAMS = (200.0, 0.72, 1.4)
BASE_T = 1.0
SPEED = 0.05


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run(n, shift, steps, warmup, say):
    import watertight_cases as W
    sh, _ = W.sphere(20, (15, 19, 15))
    g0, idx = sh.subframe(0.0)
    idx = np.asarray(idx).reshape(-1, 3)
    scale = np.array([n / sh.dimx, n / sh.dimy, n / sh.dimz])
    centre = g0.mean(axis=0, dtype=np.float64)
    total = warmup + steps
    start = -0.5 * shift * total                           # the sphere crosses the middle of the grid
    s = capi.Solver(grids.box(n, n, n), capi.fluid_params(np.float32, *PARAMS), np.float32)
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    s.enable_timing(True)
    say("grid %d^3, %.3f cells per step, %d warm-up + %d steps" % (n, shift, warmup, steps))
    say("%5s %12s %12s %14s %10s %10s %7s %6s" % ("step", "update ms", "fill ms", "fill host ms", "fresh", "filled", "rounds", "left"))
    upd, fill = [], []
    for k in range(total):
        g = (((g0 - centre) * 0.7 + centre) * scale + np.array([start + shift * k, 0.0, 0.0])).astype(np.float32)
        vel = np.zeros(g.shape, np.float32)
        vel[:, 0] = SPEED
        s.update_nodes_shape3d_vel(g, vel, idx, BASE_T, 0.0)
        t0 = time.perf_counter()
        info = s.fill_fresh_cells(capi.LAYER_CUR)          # (step 0: from the box the context was created with)
        host_ms = (time.perf_counter() - t0) * 1e3
        u, f = s.last_update_device_ms(), s.last_fill_device_ms()
        say("%5d %12.4f %12.4f %14.4f %10d %10d %7d %6d%s" % ((k, u, f, host_ms) + tuple(info) + ("  (warm-up)" if k < warmup else "",)))
        if k >= warmup:
            upd.append(u); fill.append(f)
    say("median over %d steps: update %.4f ms, fill %.4f ms (%.1f %% of the update); fill min %.4f max %.4f; allocations + frees %d\n"
        % (len(fill), median(upd), median(fill), 100.0 * median(fill) / median(upd), min(fill), max(fill),
           s.geometry_info()["device_allocs_and_frees"]))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fresh_cells_cost.txt"))
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("fs3d_fill_fresh_cells beside fs3d_update_nodes_shape3d_vel: device times in ms (HIP events inside the library), fp32, %s"
        % capi.load().fs3d_version().decode())
    for n in a.sizes:
        for shift in (0.5, n / 56.0):
            run(n, shift, a.steps, a.warmup, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
