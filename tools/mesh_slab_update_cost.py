"""What a moving Shape3D mesh costs per slab and step: fs3d_update_nodes_shape3d_slab / _vel_slab beside the path they replace.

    python tools/mesh_slab_update_cost.py [--repeats 7] [--out profiles/mesh_slab_update_cost.txt]

The 1280-face sphere watertight_cases.SINGLE[2] on its 120 x 151 x 120 grid, conservative voxelisation, fp32; the sphere and the same
shifted half a cell in x alternate.  For nranks = 1, 2, 4 the lone slab contexts of one device, one after the other (the calls talk
to no other rank, so no group is needed; nranks = 1 is the whole-grid context through the same entries), per rank the median of

    new       the device time of the entry (fs3d_last_update_device_ms) and the host clock around the call, for both entries;
              the rounds of the flood fill
    replaced  the host voxelisation of host/Shape3D.h on one thread (Build with its flood fill, FillShape3DNodes: what rank 0 of
              `fs3d_run moving-mesh --host-voxels` does while the others wait; tools/mesh_host_voxels.cpp, built here with g++),
              shown on its own, then fs3d_update_nodes_slab with those arrays: device time and host clock, copies included

Rasterisation and fill run over the global grid on every rank: that part of the new entries' device time is not expected to fall
with the number of ranks.  Needs the GPU: there is no fallback."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cmc_fluid_solver_amd import capi, grids  # noqa: E402
from cmc_fluid_solver_amd.slab import slab_range  # noqa: E402

HELPER_SRC = os.path.join(ROOT, "tools", "mesh_host_voxels.cpp")
HELPER = os.path.join(ROOT, "tools", "mesh_host_voxels")
BASE_T = 1.0


def build_helper():
    deps = [HELPER_SRC, os.path.join(ROOT, "cmc_fluid_solver_amd", "host", "Shape3D.h"), os.path.join(ROOT, "cmc_fluid_solver_amd", "csrc", "fs3d_voxel.h")]
    if not os.path.exists(HELPER) or any(os.path.getmtime(d) > os.path.getmtime(HELPER) for d in deps):
        # -ffp-contract=off: the voxel rule of csrc/fs3d_voxel.h rounds after every operation
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), HELPER_SRC, "-o", HELPER])
    return HELPER


def host_voxels(dims, g, vel, idx, repeats):
    """(Nodes of the host voxelisation, Build ms per repeat, FillShape3DNodes ms per repeat); vel None: walls at rest"""
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        with open(fin, "wb") as f:
            np.array(list(dims) + [len(g), len(idx), int(vel is not None), repeats], np.int32).tofile(f)
            for a in (g,) if vel is None else (g, vel):
                for c in range(3):
                    np.ascontiguousarray(a[:, c], np.float32).tofile(f)
            np.ascontiguousarray(idx, np.int32).tofile(f)
        out = subprocess.run([build_helper(), fin, fout], capture_output=True, text=True, check=True).stdout
        n = int(np.prod(dims))
        raw = np.fromfile(fout, np.uint8)
    by = [raw[q * n:(q + 1) * n].reshape(dims).copy() for q in range(3)]
    va = [raw[3 * n:].view(np.float32)[q * n:(q + 1) * n].reshape(dims).astype(np.float64) for q in range(4)]
    ms = {l.split()[0]: [float(x) for x in l.split()[1:]] for l in out.splitlines()}
    return grids.Nodes(dims[0], dims[1], dims[2], 0.001, 0.001, 0.001, *by, *va), ms["BUILD_MS"], ms["NODES_MS"]


def med(v):
    return statistics.median(v)


def measure(s, calls, repeats):
    """calls: the two alternating geometries as callables -> (median device ms, median host ms)"""
    for k in (1, 0, 1, 0):                                  # warm-up: first launches, the buffers the first updates allocate
        calls[k]()
    host, dev = [], []
    for r in range(repeats):
        t0 = time.perf_counter(); calls[(r + 1) % 2](); s.synchronize()
        host.append((time.perf_counter() - t0) * 1e3); dev.append(s.last_update_device_ms())
    return med(dev), med(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_slab_update_cost.txt"))
    a = ap.parse_args()
    import wall_velocity_cases as WV
    import watertight_cases as W
    faces, r, dims = W.SINGLE[2]
    sh, _ = W.sphere(faces, r)
    assert sh.type.shape == dims
    g0, idx = sh.subframe(0.0)
    g0, idx = np.asarray(g0, np.float32), np.asarray(idx).reshape(-1, 3)
    meshes = [g0, (g0 + np.array([0.5, 0.0, 0.0], np.float32)).astype(np.float32)]
    vels = [(WV.velocities(g) * np.float32(2.0 ** -10)).astype(np.float32) for g in meshes]
    params = capi.fluid_params(np.float32, 200.0, 0.72, 1.4)
    lines = ["mesh: %d faces, %d vertices; grid %d x %d x %d (%d cells), conservative voxelisation, fp32; medians of %d calls, ms"
             % (len(idx), len(g0), dims[0], dims[1], dims[2], int(np.prod(dims)), a.repeats)]
    host = {}
    for tag, vv in (("plain", [None, None]), ("vel", vels)):
        res = [host_voxels(dims, g, v, idx, a.repeats) for g, v in zip(meshes, vv)]
        host[tag] = [x[0] for x in res]
        lines.append("host voxelisation, one thread (%s): Build + flood fill %.3f, FillShape3DNodes %.3f" %
                     ("walls at rest" if tag == "plain" else "with wall velocities", med(res[0][1] + res[1][1]), med(res[0][2] + res[1][2])))
    assert np.array_equal(host["plain"][0].type, sh.type)                       # the helper and the twin agree on the grid
    lines.append("per rank: device ms / host-clock ms of the call")
    for nranks in (1, 2, 4):
        for rank in range(nranks):
            xr = slab_range(dims[0], rank, nranks)
            s = capi.Solver(host["plain"][0], params, np.float32, x_range=xr)
            s.set_option(capi.OPT_MESH_VOXELS, 1)
            s.enable_timing(True)
            row = {}
            row["shape3d_slab"] = measure(s, [lambda g=g: s.update_nodes_shape3d_slab(g, idx, BASE_T) for g in meshes], a.repeats)
            rounds = s.mesh_fill_rounds()
            row["shape3d_vel_slab"] = measure(s, [lambda g=g, v=v: s.update_nodes_shape3d_vel_slab(g, v, idx, BASE_T, 0.0) for g, v in zip(meshes, vels)], a.repeats)
            row["update_nodes_slab (walls at rest)"] = measure(s, [lambda n=n: s.update_nodes_slab(n) for n in host["plain"]], a.repeats)
            row["update_nodes_slab (wall velocities)"] = measure(s, [lambda n=n: s.update_nodes_slab(n) for n in host["vel"]], a.repeats)
            s.close()
            lines.append("nranks %d rank %d planes %3d..%3d: new " % (nranks, rank, xr[0], xr[1]) +
                         ", ".join("%s %.3f / %.3f" % (k, *row[k]) for k in ("shape3d_slab", "shape3d_vel_slab")) +
                         " (fill rounds %d); replaced, after the host voxelisation above: " % rounds +
                         ", ".join("%s %.3f / %.3f" % (k, *row[k]) for k in ("update_nodes_slab (walls at rest)", "update_nodes_slab (wall velocities)")))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
