"""What the collective fresh-cell fill (FS3D_OPT_FRESH_CELLS_SLABS) costs on x-slabs, beside the single context's fill.

    python tools/fresh_cells_slab_cost.py [--sizes 128 256] [--groups 1 2 4] [--steps 20] [--warmup 3] [--out profiles/fresh_cells_slab_cost.txt]

The sphere of tools/fresh_cells_cost.py (20 faces, walls at the mesh's velocity and temperature 0, conservative voxelisation) at N^3,
fp32, its two motions (half a cell per step; N / 56 cells per step: a thicker shell, several rounds).  First a single context
(fs3d_update_nodes_shape3d_vel, fs3d_fill_fresh_cells): the yardstick, from the same process.  Then in-process groups of 1, 2 and 4
x-slabs on ONE card, one host thread per slab (fs3d_update_nodes_shape3d_vel_slab, the collective fs3d_fill_fresh_cells).  Per rank,
the median over the steps after the warm-up of: the fill's device time (fs3d_last_fill_device_ms: the rank's own kernels and copies,
the snapshot's copy kernel included; the transport's copies and waits are not in it) and the host clock around the fill call, which
is what the caller waits.  The exchanges are counted from the protocol: one grouped exchange before every round launched, rounds
launched in batches of 2 until the first round that fills nothing on any rank or the last fresh cell, one sum over the ranks after
the classifying pass and one per batch.
The host clock of the in-process transport -- two stream synchronisations and a rendezvous of host threads per exchange, the slabs
sharing one card -- says nothing about RCCL ranks on several cards: that number remains unmeasured.
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
BATCH = 2                                                  # FRESH_BATCH of csrc/kernels_geom.hip


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def meshes(n, shift, total):
    """[(vertices, velocities)] per step and the triangles: the motion of tools/fresh_cells_cost.py"""
    import watertight_cases as W
    sh, _ = W.sphere(20, (15, 19, 15))
    g0, idx = sh.subframe(0.0)
    idx = np.asarray(idx).reshape(-1, 3)
    scale = np.array([n / sh.dimx, n / sh.dimy, n / sh.dimz])
    centre = g0.mean(axis=0, dtype=np.float64)
    start = -0.5 * shift * total                           # the sphere crosses the middle of the grid
    out = []
    for k in range(total):
        g = (((g0 - centre) * 0.7 + centre) * scale + np.array([start + shift * k, 0.0, 0.0])).astype(np.float32)
        vel = np.zeros(g.shape, np.float32)
        vel[:, 0] = SPEED
        out.append((g, vel))
    return out, idx


def loop(s, steps, idx, update):
    """[(fill device ms, fill host ms, info)] per step on one context (a slab thread of a group, or the single context)"""
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    s.enable_timing(True)
    rec = []
    for g, vel in steps:
        update(g, vel, idx, BASE_T, 0.0)
        t0 = time.perf_counter()
        info = s.fill_fresh_cells(capi.LAYER_CUR)
        host_ms = (time.perf_counter() - t0) * 1e3
        rec.append((s.last_fill_device_ms(), host_ms, info))
    return rec


def exchanges(infos):
    """(grouped exchanges per rank that has a neighbour, sums over the ranks) of one collective fill, from every rank's info"""
    fresh, filled, rounds = sum(i[0] for i in infos), sum(i[1] for i in infos), infos[0][2]
    if fresh == 0:
        return 0, 1
    last = rounds if filled == fresh else rounds + 1      # the round whose count ends the fill
    launched = min(250, (last + BATCH - 1) // BATCH * BATCH)
    return launched, 1 + (launched + BATCH - 1) // BATCH


def run(n, shift, groups, nsteps, warmup, say):
    steps, idx = meshes(n, shift, warmup + nsteps)
    nodes = grids.box(n, n, n)
    params = capi.fluid_params(np.float32, *PARAMS)
    say("grid %d^3, %.3f cells per step, %d warm-up + %d steps" % (n, shift, warmup, nsteps))
    s = capi.Solver(nodes, params, np.float32)
    rec = loop(s, steps, idx, s.update_nodes_shape3d_vel)[warmup:]
    s.close()
    single = median([r[0] for r in rec])
    say("  single context       : fill device %.4f ms, host clock %.4f ms; fresh %d .. %d, rounds %d .. %d" % (
        single, median([r[1] for r in rec]), min(r[2][0] for r in rec), max(r[2][0] for r in rec), min(r[2][2] for r in rec), max(r[2][2] for r in rec)))
    for nranks in groups:
        grp = capi.LocalGroup(nodes, params, nranks, np.float32)
        for q in grp.solvers:
            q.set_option(capi.OPT_FRESH_CELLS_SLABS, 1)
        res = grp.run(lambda rank, q: loop(q, steps, idx, q.update_nodes_shape3d_vel_slab))
        allocs = [q.geometry_info()["device_allocs_and_frees"] for q in grp.solvers]
        grp.close()
        ex = [exchanges([res[r][k][2] for r in range(nranks)]) for k in range(warmup, warmup + nsteps)]
        for r in range(nranks):
            mine = res[r][warmup:]
            say("  %d slabs, rank %d       : fill device %.4f ms (%.2f x single), host clock %.4f ms; own fresh %d .. %d; exchanges %d .. %d, sums %d .. %d%s" % (
                nranks, r, median([m[0] for m in mine]), median([m[0] for m in mine]) / single, median([m[1] for m in mine]),
                min(m[2][0] for m in mine), max(m[2][0] for m in mine), min(e[0] for e in ex) if nranks > 1 else 0,
                max(e[0] for e in ex) if nranks > 1 else 0, min(e[1] for e in ex), max(e[1] for e in ex),
                "; allocations + frees %d" % allocs[r] if r == 0 else ""))
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fresh_cells_slab_cost.txt"))
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("collective fs3d_fill_fresh_cells on in-process x-slabs of one card beside the single context's fill: medians over the steps, ms, fp32, %s"
        % capi.load().fs3d_version().decode())
    say("(device: HIP events inside the library around the rank's own kernels and copies; host clock: around the call, with the in-process")
    say(" transport's stream synchronisations and thread rendezvous per exchange -- no statement about RCCL ranks)")
    for n in a.sizes:
        for shift in (0.5, n / 56.0):
            run(n, shift, a.groups, a.steps, a.warmup, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
