"""What a change of geometry costs per call, and whether a time step runs as fast on updated tables as on uploaded ones.

    python tools/geometry_update_cost.py [--repeats 20] [--out profiles/geometry_update_cost.json]

Two cases: the heart_us grid (96 x 160 x 128, two geometries of its cycle) and the 256^3 masked case (the non_uniform256 nodes and
the same with a solid block added).  Per case, alternating the two geometries after a warm-up:
  (a) fs3d_upload_nodes per call       -- host clock around the call (it ends synchronised): the only way before fs3d_update_nodes
  (b) fs3d_update_nodes per call       -- host arrays, copies included; host clock
  (c) fs3d_update_nodes_dev per call   -- device arrays; host clock, and the device time alone (HIP events inside the library)
  (d) time per step (G 4, L 2, AUTO, fp32) after an upload and after an update of the same geometry, interleaved, with the spread
Needs the GPU: there is no fallback.  One process, one context per case.

    python tools/geometry_update_cost.py --extrude [--repeats 20] [--out profiles/extrude_update_cost.json] [--kernel-trace CSV]

The extrusion of a Shape2D grid on the device (fs3d_update_nodes_shape2d) against today's path, on heart_us at the shipped resolution
(96 x 160 x 128) and at grid_dx 0.00027, grid_dz 0.004 (256 x 384 x 256).  Per grid, two geometries of the cycle alternating, interleaved
in one process, after a warm-up:
  (e) fs3d_update_nodes per call          -- the host-extruded node arrays, copies included; host clock
  (f) fs3d_update_nodes_shape2d per call  -- the 2D grid; host clock, and the device time alone
  (g) the driver, `moving` and `moving --host-extrusion`, alternating: per step the host clock around Grid2D::Prepare, the host
      ExtrudeShape2D and the update call, and the whole step (fs3d_run --time-geometry)
  (h) k_geom_extrude alone, against its bytes (19 per cell) and the box's write-only rate (5.4 TB/s, profiles/r3_stream_ubench2.txt),
      from a second run of the library calls under the profiler.  Three steps:
        1. python tools/geometry_update_cost.py --extrude                                   -> profiles/extrude_update_cost.json, rows (e)-(g)
        2. rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ext -- \
               python tools/geometry_update_cost.py --extrude --skip-driver                 -> DIR/ext_kernel_trace.csv, DIR/ext_kernel_stats.csv
           (--skip-driver: no child processes under the profiler; its own rows are printed, and written only where --out names a file)
        3. python tools/geometry_update_cost.py --extrude --kernel-trace DIR/ext_kernel_trace.csv
           adds the kernel rows to the file of step 1, which must exist; DIR/ext_kernel_stats.csv is kept as profiles/extrude_kernel_stats.csv

    python tools/geometry_update_cost.py --mesh [--out profiles/mesh_update_cost.json] [--write-inputs DIR] [--kernel-stats CSV]

    python tools/geometry_update_cost.py --mesh --voxels conservative [--out profiles/mesh_update_cost_conservative.json]
        (the conservative voxelisation, FS3D_OPT_MESH_VOXELS = 1, beside the default one on the same two grids: main_mesh_voxels;
        kernel rows: --kernel-stats CSV of a rocprofv3 --kernel-trace --stats run of `fs3d_run ... moving-mesh --watertight`)

    python tools/geometry_update_cost.py --mesh --voxels conservative --shell box|cross [--repeats 24] [--out FILE]
        (the thin shell, FS3D_OPT_MESH_SHELL = 1, against the conservative shell: main_mesh_shell -- ONE configuration per process, the
        1280-face sphere watertight_cases.SINGLE[2] on its 120 x 151 x 120 grid breathing between x 1.0 and x 0.95, device time of
        fs3d_update_nodes_shape3d after 4 warm-up calls; one line of JSON, appended to FILE where --out names one.  `box` never touches
        the option, so FS3D_LIB_PATH may name the library of a commit that does not have it: run fresh processes alternating,
        profiles/mesh_thin_shell_cost.txt)

A moving Shape3D mesh: the voxelisation and flood fill on the device (fs3d_update_nodes_shape3d) against today's path.  The mesh is an
icosphere of 1280 faces (642 vertices; the reference's heart_us_3D has 1294 triangles) breathing between two radii (x 1.0 and x 0.9), stretched to fill a
grid of heart_us_3D's size, 128 x 160 x 128, and one of 256^3.  Everything runs in the driver, fs3d_run ... moving-mesh:
  (a) Shape3D::Prepare(t) on the host + fs3d_update_nodes   and   (b) fs3d_update_nodes_shape3d, both per step of ONE process
      (--time-both: host clock around each, the device time of (b), the time step of the same steps), after 3 warm-up steps
  (c) the whole step of `moving-mesh` and of `moving-mesh --host-voxels`, runs alternating (--time-geometry)
  (d) the kernels of (b) by name, from a run of the driver under the profiler:
        1. python tools/geometry_update_cost.py --mesh --write-inputs DIR       the mesh and config files, nothing else
        2. rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o mesh -- \
               cmc_fluid_solver_amd/fs3d_run DIR/<grid>_data.txt OUT/run DIR/<grid>_config.txt align GPU moving-mesh --steps 12
        3. python tools/geometry_update_cost.py --mesh --kernel-stats OUT/mesh_kernel_stats.csv --grid <grid>
           adds the rows to the file of the --mesh run, which must exist
"""
import argparse
import copy
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


WRITE_ONLY_TBS = 5.4          # profiles/r3_stream_ubench2.txt


def heart_config(dx=None, dz=None):
    """The shipped heart_us config, optionally at another resolution; returns the path of a temporary copy."""
    import tempfile
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "heart_us_2D_config.txt")).read()
    out = []
    for ln in text.splitlines():
        w = ln.split()
        if dx is not None and w and w[0] in ("grid_dx", "grid_dy"):
            ln = "%s %r" % (w[0], dx)
        if dz is not None and w and w[0] == "grid_dz":
            ln = "%s %r" % (w[0], dz)
        out.append(ln)
    f = tempfile.NamedTemporaryFile("w", suffix="_config.txt", delete=False)
    f.write("\n".join(out) + "\n")
    f.close()
    return f.name


def measure_extrude(name, cfgf, repeats, driver_steps=12, driver_runs=5, skip_driver=False):
    import re
    from cmc_fluid_solver_amd import build as B
    from cmc_fluid_solver_amd import shape2d
    dtype = np.float32
    data = os.path.join(ROOT, "tests", "golden", "inputs", "heart_us_2D_data.txt")
    cfg = shape2d.Config(cfgf)
    ex = (cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT)
    g2s, nodes = [], []
    cyc = None
    for frac in (0.0, 0.37):
        g2 = shape2d.Grid2D(shape2d.parse_shape2d(open(data).read()), cfg.dx, cfg.dy, cfg.baseT, True, 0.0)
        cyc = g2.cycle_length()
        g2.prepare(frac * cyc)
        g2s.append(g2)
        nodes.append(shape2d.extrude_grid2d(g2, *ex, align=True))
    s = capi.Solver(nodes[0], capi.fluid_params(dtype, cfg.Re, cfg.Pr, cfg.lam), dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_AUTO)
    host = [arrays(n, dtype) for n in nodes]
    nseg = (C.c_int * 3)()

    def update(k):
        s._chk(s.lib.fs3d_update_nodes(s.h, *[capi._p(a) for a in host[k]], nseg))

    def update_2d(k):
        s.update_nodes_shape2d(g2s[k], *ex)

    def clock(fn, k):
        t0 = time.perf_counter(); fn(k); s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"dims": list(nodes[0].shape), "cells": nodes[0].ncells, "columns": g2s[0].dimx * g2s[0].dimy,
           "bytes_per_call_update_nodes": 19 * nodes[0].ncells, "bytes_per_call_update_nodes_shape2d": 13 * g2s[0].dimx * g2s[0].dimy}
    info = {}
    for fn in (update, update_2d):
        for k in (1, 0, 1):
            fn(k)
        info[fn.__name__] = s.geometry_info()
    out["tables_equal"] = all(info["update"][k] == info["update_2d"][k] for k in capi.Solver.GEOMETRY_INFO[:13])
    s.enable_timing(True)
    t_up, t_2d, d_up, d_2d = [], [], [], []
    for r in range(repeats):                                 # interleaved: both paths see the same box in the same minute
        k = r % 2
        t_up.append(clock(update, k)); d_up.append(s.last_update_device_ms())
        t_2d.append(clock(update_2d, k)); d_2d.append(s.last_update_device_ms())
    s.enable_timing(False)
    out["update_nodes"], out["update_nodes_device_time"] = stats(t_up), stats(d_up)
    out["update_nodes_shape2d"], out["update_nodes_shape2d_device_time"] = stats(t_2d), stats(d_2d)
    out["shape2d_over_update_nodes"] = out["update_nodes_shape2d"]["median_ms"] / out["update_nodes"]["median_ms"]
    out["condition_1_shape2d_call_faster"] = out["update_nodes_shape2d"]["median_ms"] < out["update_nodes"]["median_ms"]
    s.close()
    if skip_driver:
        print(name, json.dumps(out), flush=True)
        return out
    # the driver, both words alternating
    driver = B.build_driver()
    keys = ("prepare_ms", "host_extrusion_ms", "update_call_ms", "step_ms")
    runs = {"moving": {k: [] for k in keys}, "moving --host-extrusion": {k: [] for k in keys}}
    for r in range(driver_runs + 1):
        for word in runs:
            o = subprocess.run([driver, data, "/tmp/extrude_cost_%d" % os.getpid(), cfgf, "align", "GPU"] + word.split() + ["--time-geometry", "--steps", str(driver_steps)],
                               check=True, capture_output=True, text=True, timeout=900).stdout
            m = re.search(r"Prepare ([0-9.]+), extrusion on the host ([0-9.]+), update call ([0-9.]+); step ([0-9.]+)", o)
            if r:                                            # the first pair is the warm-up
                for k, v in zip(keys, m.groups()):
                    runs[word][k].append(float(v))
    out["driver"] = {w: {k: stats(v) for k, v in d.items()} for w, d in runs.items()}
    out["driver"]["steps_per_run"] = driver_steps
    dm, dh = out["driver"]["moving"]["step_ms"], out["driver"]["moving --host-extrusion"]["step_ms"]
    out["condition_2_driver_step_faster"] = dm["median_ms"] < dh["median_ms"]
    out["driver_step_host_over_device"] = dh["median_ms"] / dm["median_ms"]
    for f in ("/tmp/extrude_cost_%d_res.nc" % os.getpid(),):
        if os.path.exists(f):
            os.unlink(f)
    print(name, json.dumps(out), flush=True)
    return out


def kernel_rows(csv_path, cells_by_grid):
    """k_geom_extrude dispatches of a rocprofv3 kernel trace, by grid: median duration against 19 bytes per cell."""
    import csv
    by = {}
    for row in csv.DictReader(open(csv_path)):
        if "k_geom_extrude" not in row.get("Kernel_Name", ""):
            continue
        threads = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
        by.setdefault(threads, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = {}
    for threads, us in sorted(by.items()):
        cells = min(cells_by_grid, key=lambda c: abs(c / 4 - threads))       # one thread per 4 cells, rounded up to workgroups of 256
        st = {"n": len(us), "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "cells": cells, "bytes": 19 * cells}
        st["TB_per_s"] = st["bytes"] / (st["median_us"] * 1e-6) / 1e12
        st["fraction_of_write_only_rate"] = st["TB_per_s"] / WRITE_ONLY_TBS
        out["%s (%d threads)" % (cells_by_grid[cells], threads)] = st
    return out


def main_extrude(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "extrude_update_cost.json")
    if a.skip_driver and a.out == DEFAULT_OUT:
        out_path = None                                      # the run under the profiler never replaces the complete file
    if a.kernel_trace and not (os.path.exists(out_path) and "driver" in json.load(open(out_path)).get("heart_us", {})):
        raise SystemExit("--kernel-trace: %s does not hold the rows of a complete --extrude run (step 1)" % out_path)
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or tree_commit(), "repeats": a.repeats, "precision": "fp32",
           "note": "host clock around calls that end synchronised, the two paths interleaved; device time from HIP events inside the library; "
                   "driver: fs3d_run --time-geometry, 12 steps per run, the two words alternating"}
    if a.kernel_trace:                                       # the kernel rows come from a second run, under the profiler
        res = json.load(open(out_path))
    else:
        shipped, fine = heart_config(), heart_config(dx=0.00027, dz=0.004)
        res["heart_us"] = measure_extrude("heart_us", shipped, a.repeats, skip_driver=a.skip_driver)
        res["heart_us_256x384x256"] = measure_extrude("heart_us_256x384x256", fine, a.repeats, driver_runs=3, skip_driver=a.skip_driver)
        os.unlink(shipped); os.unlink(fine)
    if a.kernel_trace:
        res["k_geom_extrude"] = kernel_rows(a.kernel_trace, {res[k]["cells"]: k for k in ("heart_us", "heart_us_256x384x256")})
        res["k_geom_extrude"]["write_only_rate_TB_per_s"] = WRITE_ONLY_TBS
    if out_path is None:
        return
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


# radii in mm (cells).  The reference's rasteriser leaves holes in some meshes (the flood fill then takes the inside as well): these
# two stay closed at every time of the run, which the run checks through its NODE_IN count
MESH_GRIDS = {"heart_size_128x160x128": ((52.0, 66.0, 52.0), (128, 160, 128)), "cube_256": ((118.0, 118.0, 118.0), (256, 256, 256))}
MESH_CONFIG = """dimension 3D
in_fmt Shape3D
Re 200.0
Pr 0.72
lambda 1.4
bc_type NoSlip
grid_dx 0.001
grid_dy 0.001
grid_dz 0.001
frame_time 0.4
cycles 1
time_steps 16
out_time_steps 1000
out_gridx 16
out_gridy 16
out_gridz 16
out_fmt NetCDF
out_vars 4 u v w T
solver ADI
num_global 4
num_local 2
"""


def write_mesh_inputs(d):
    """Per grid: an icosphere of 1280 faces stretched to the radii (mm), and the same at 0.9 of them as the second frame."""
    from cmc_fluid_solver_amd import shape3d
    from test_shape3d import icosphere
    out = {}
    os.makedirs(d, exist_ok=True)
    for name, (radii, dims) in MESH_GRIDS.items():
        v, f = icosphere(1.0, (0.0, 0.0, 0.0), subdiv=3)
        assert len(f) == 1280
        centre = np.array(radii) * 1.5 + 0.5
        frames = [(v * np.array(radii) * k + centre, f) for k in (1.0, 0.9)]
        data, cfg = os.path.join(d, name + "_data.txt"), os.path.join(d, name + "_config.txt")
        shape3d.write_mesh(data, frames)
        open(cfg, "w").write(MESH_CONFIG)
        out[name] = (data, cfg, dims)
    return out


def main_mesh(a):
    import re
    import tempfile
    from cmc_fluid_solver_amd import build as B
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "mesh_update_cost_conservative.json" if a.voxels else "mesh_update_cost.json")
    if a.write_inputs:
        for name, (data, cfg, dims) in write_mesh_inputs(a.write_inputs).items():
            print(name, data, cfg)
        return
    if a.kernel_stats:
        import csv
        res = json.load(open(out_path))
        rows = {}
        for row in csv.DictReader(open(a.kernel_stats)):
            nm = row["Name"].split("(")[0]
            if "k_geom_" in nm or "k_clear_outer" in nm:
                rows[nm] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3, "average_us": float(row["AverageNs"]) / 1e3}
        part = lambda pred: sum(r["total_us"] for n, r in rows.items() if pred(n))
        updates = rows[[n for n in rows if "k_geom_codes" in n][0]]["calls"]
        res[a.grid]["kernels"] = {"rows": rows, "updates": updates,
                                  "raster_us_per_update": part(lambda n: "raster_mesh" in n) / updates,
                                  "voxel_us_per_update": part(lambda n: "voxel_mesh" in n) / updates,
                                  "fill_us_per_update": part(lambda n: "k_geom_fill" in n) / updates,
                                  "node_arrays_us_per_update": part(lambda n: "mesh_nodes" in n) / updates,
                                  "table_rebuild_us_per_update": part(lambda n: "k_geom_" in n and "raster" not in n and "voxel_mesh" not in n and "fill" not in n and "mesh_nodes" not in n) / updates}
        json.dump(res, open(out_path, "w"), indent=1)
        print(json.dumps(res[a.grid]["kernels"], indent=1))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    driver = B.build_driver()
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or tree_commit(), "precision": "fp32",
           "mesh": "icosphere, 1280 faces, 642 vertices, two frames (radii x 1.0 and x 0.9)",
           "note": "fs3d_run moving-mesh; (a)/(b): --time-both, both paths in every step of one process, 3 warm-up steps dropped, host clock around "
                   "calls that end synchronised, device time from HIP events inside the library; (c): --time-geometry, runs alternating"}
    num = r"median ([0-9.]+) min ([0-9.]+) max ([0-9.]+) n (\d+)"
    with tempfile.TemporaryDirectory() as d:
        for name, (data, cfg, dims) in write_mesh_inputs(d).items():
            base = [driver, data, os.path.join(d, "run"), cfg, "align", "GPU", "moving-mesh"]
            o = subprocess.run(base + ["--time-both", "--steps", str(a.repeats + 3)], check=True, capture_output=True, text=True, timeout=1200).stdout
            got = tuple(int(x) for x in re.search(r"Grid = (\d+) x (\d+) x (\d+)", o).groups())
            assert got == dims, (got, dims)
            assert float(re.search(r"NODE_IN points = ([0-9.]+)", o).group(1)) > got[0] * got[1] * got[2] / 8, "the mesh is not closed"
            r = {"dims": list(got), "cells": got[0] * got[1] * got[2], "fill_rounds": int(re.search(r"fill rounds (\d+)", o).group(1))}
            for key, label in (("a_host_voxels_update_nodes", "host voxels \\+ fs3d_update_nodes"), ("b_update_nodes_shape3d", "fs3d_update_nodes_shape3d"),
                               ("b_device_time", "its device time"), ("time_step", "time step")):
                m = re.search(label + " " + num, o)
                r[key] = {"median_ms": float(m.group(1)), "min_ms": float(m.group(2)), "max_ms": float(m.group(3)), "n": int(m.group(4))}
            r["b_over_a"] = r["b_update_nodes_shape3d"]["median_ms"] / r["a_host_voxels_update_nodes"]["median_ms"]
            r["condition_b_below_a_ranges_apart"] = r["b_update_nodes_shape3d"]["max_ms"] < r["a_host_voxels_update_nodes"]["min_ms"]
            r["b_device_time_over_time_step"] = r["b_device_time"]["median_ms"] / r["time_step"]["median_ms"]
            runs = {"moving-mesh": [], "moving-mesh --host-voxels": []}
            for k in range(a.driver_runs + 1):
                for word, acc in runs.items():
                    o = subprocess.run(base + word.split()[1:] + ["--time-geometry", "--steps", "12"], check=True, capture_output=True, text=True, timeout=1200).stdout
                    if k:                                    # the first pair is the warm-up
                        acc.append(float(re.search(r"update call [0-9.]+; step ([0-9.]+)", o).group(1)))
            r["driver_step"] = {w: stats(v) for w, v in runs.items()}
            r["condition_driver_step_not_above_host_voxels"] = r["driver_step"]["moving-mesh"]["median_ms"] <= r["driver_step"]["moving-mesh --host-voxels"]["median_ms"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def main_mesh_voxels(a):
    """--mesh --voxels conservative: the two grids of --mesh, fs3d_update_nodes_shape3d with FS3D_OPT_MESH_VOXELS 0 and 1 alternating
    in one process (the mesh breathes between its two frames, one update per mode and sample), then the time step of the same
    geometry.  Condition: the conservative update's device time stays below the time step, on both grids."""
    import tempfile
    import torch
    from cmc_fluid_solver_amd import shape3d
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    out_path = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "mesh_update_cost_conservative.json")
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or tree_commit(), "precision": "fp32", "repeats": a.repeats,
           "mesh": "icosphere, 1280 faces, 642 vertices, two frames (radii x 1.0 and x 0.9)",
           "note": "one process per grid; per sample one fs3d_update_nodes_shape3d per mode (default first), alternating, 3 warm-up samples "
                   "dropped; host clock around calls that end synchronised, device time from HIP events inside the library; step = G 4, L 2, AUTO"}
    h = float(np.float32(0.001))
    with tempfile.TemporaryDirectory() as d:
        for name, (data, cfg, dims) in write_mesh_inputs(d).items():
            nodes, sh = shape3d.load_shape3d(data, h, h, h, align=True, voxels="conservative")
            assert nodes.shape == dims, (nodes.shape, dims)
            s = capi.Solver(nodes, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)
            s.enable_timing(True)
            acc = {m: {"host": [], "dev": [], "fluid": None} for m in ("reference", "conservative")}
            step = []
            for k in range(a.repeats + 3):
                g, idx = sh.subframe(0.4 / 2 * ((k % 16) / 16.0))
                for m in ("reference", "conservative"):
                    t0 = time.perf_counter()
                    s.update_nodes_shape3d(g, idx, 1.0, voxels=m)
                    ms = (time.perf_counter() - t0) * 1e3
                    if k >= 3:
                        acc[m]["host"].append(ms); acc[m]["dev"].append(s.last_update_device_ms())
                    info = s.geometry_info()
                    acc[m]["fluid"] = int(np.prod(dims)) - info["bound_cells"]
                    acc[m]["fill_rounds"] = s.mesh_fill_rounds()
                t0 = time.perf_counter()
                s.UpdateBoundaries(); s.TimeStep(np.float32(0.4 / 32), 4, 2, False)
                s._chk(s.lib.fs3d_synchronize(s.h))
                if k >= 3:
                    step.append((time.perf_counter() - t0) * 1e3)
            s.close()
            r = {"dims": list(dims), "cells": int(np.prod(dims)), "time_step": stats(step)}
            for m in acc:
                r[m] = {"update_nodes_shape3d": stats(acc[m]["host"]), "device_time": stats(acc[m]["dev"]), "fill_rounds": acc[m]["fill_rounds"]}
            r["conservative_device_time_over_time_step"] = r["conservative"]["device_time"]["median_ms"] / r["time_step"]["median_ms"]
            r["conservative_over_reference_device_time"] = r["conservative"]["device_time"]["median_ms"] / r["reference"]["device_time"]["median_ms"]
            r["condition_conservative_device_time_below_time_step"] = r["conservative"]["device_time"]["median_ms"] < r["time_step"]["median_ms"]
            res[name] = r
            print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


def main_mesh_shell(a):
    """--mesh --voxels conservative --shell box|cross: one configuration, one process, one line of JSON."""
    import torch
    import watertight_cases as W
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    faces, r, dims = W.SINGLE[2]
    sh, _ = W.sphere(faces, r)
    g0, idx = sh.subframe(0.0)
    centre = g0.mean(axis=0, dtype=np.float64)
    meshes = [((g0 - centre) * k + centre).astype(np.float32) for k in (1.0, 0.95)]
    nodes = shape3d_nodes(sh)
    assert nodes.shape == dims, (nodes.shape, dims)
    s = capi.Solver(nodes, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)
    s.enable_timing(True)
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    if a.shell == "cross":
        s.set_option(capi.OPT_MESH_SHELL, 1)
    dev, host = [], []
    for k in range(a.repeats + 4):
        t0 = time.perf_counter()
        s.update_nodes_shape3d(meshes[k % 2], idx, 1.0)
        ms = (time.perf_counter() - t0) * 1e3
        if k >= 4:
            dev.append(s.last_update_device_ms()); host.append(ms)
    info = s.geometry_info()
    tw = copy.copy(sh)                                       # the twin's grid of the last mesh: the fluid cells, and a check of the shell
    tw.voxels, tw.shell = "conservative", a.shell
    tw.build(meshes[(a.repeats + 3) % 2], idx)
    assert info["bound_cells"] == int((tw.type == grids.NODE_BOUND).sum()), "the device's shell is not the twin's"
    r = {"device": torch.cuda.get_device_name(0), "commit": a.commit or tree_commit(), "library": capi.LIB_PATH, "shell": a.shell,
         "dims": list(dims), "faces": faces, "device_time": stats(dev), "update_nodes_shape3d": stats(host),
         "bound_cells": info["bound_cells"], "fluid_cells": int((tw.type == grids.NODE_IN).sum()),
         "fill_rounds": s.mesh_fill_rounds()}
    s.close()
    line = json.dumps(r)
    print(line, flush=True)
    if a.out != DEFAULT_OUT:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def shape3d_nodes(sh):
    from cmc_fluid_solver_amd import shape3d
    return shape3d.nodes_of(sh, sh.dx, sh.dy, sh.dz, 1.0)


def tree_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


DEFAULT_OUT = os.path.join(ROOT, "profiles", "geometry_update_cost.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--extrude", action="store_true", help="the rows of the device extrusion (profiles/extrude_update_cost.json)")
    ap.add_argument("--skip-driver", action="store_true", help="--extrude: the library calls only (the run under the profiler)")
    ap.add_argument("--kernel-trace", default=None, help="--extrude: ..._kernel_trace.csv of a rocprofv3 run of this command; adds the kernel rows")
    ap.add_argument("--mesh", action="store_true", help="the rows of the device voxeliser of Shape3D meshes (profiles/mesh_update_cost.json)")
    ap.add_argument("--voxels", default=None, choices=["conservative"],
                    help="--mesh: the conservative voxelisation beside the default one (profiles/mesh_update_cost_conservative.json)")
    ap.add_argument("--shell", default=None, choices=["box", "cross"],
                    help="--mesh --voxels conservative: one configuration of the thin-shell comparison (profiles/mesh_thin_shell_cost.txt)")
    ap.add_argument("--write-inputs", default=None, help="--mesh: write the mesh and config files of the two grids into this directory and stop")
    ap.add_argument("--kernel-stats", default=None, help="--mesh: ..._kernel_stats.csv of a rocprofv3 run of the driver; adds the kernel rows of --grid")
    ap.add_argument("--grid", default="heart_size_128x160x128", help="--mesh --kernel-stats: the grid the profiled run used")
    ap.add_argument("--driver-runs", type=int, default=3, help="--mesh: runs per word of row (c), after one warm-up pair")
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse of the tree)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if a.extrude:
        return main_extrude(a)
    if a.mesh and a.voxels and a.shell:
        return main_mesh_shell(a)
    if a.mesh and a.voxels and not a.kernel_stats and not a.write_inputs:
        return main_mesh_voxels(a)
    if a.mesh:
        return main_mesh(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("geometry_update_cost: no GPU (there is no CPU fallback)")
    torch.cuda.init()                       # torch opens the device before the library does (its tensors are handed to the library)
    import refgolden as RG
    from cmc_fluid_solver_amd import shape2d
    commit = a.commit or tree_commit()
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
