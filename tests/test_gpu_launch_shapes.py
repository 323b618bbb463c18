"""Every launch shape of the partition sweep kernels on the GPU, each on the smallest grid that reaches it: the table of
tests/launch_shape_cases.py (its CPU conditions: tests/test_launch_shape_cases.py) against the CPU oracle, through the C ABI.

The host dispatch picks one of 35 template instances of k_sweep_part / k_sweep_part_z, a workgroup order and a number of rows per
wave from the grid's dimensions alone.  Per entry, under FS3D_SWEEP_PART (fp64: FS3D_OPT_F64_PART = 1), an unmerged sweep of the
entry's direction with the sentinel in next, then the merged sweep:
    the launch            last_sweep_kernels() says "part" and last_sweep_launch() is the entry's record field by field (slabs: both
                          passes on every rank): an entry cannot pass on another instance than the one it is there for
    the written cells     the oracle's; temp untouched without the merge, cells that are not NODE_IN untouched with it
    rel-L2 per field      <= TOL_SWEEP of tests/test_gpu_part.py (fp64: x SCALE of tests/test_gpu_part_f64.py)
    per LINE              bc_cases.check_lines as it stands, on next and on the merged temp: over the cells the fp64 oracle wrote,
                          S = max |x64| per field, e(K) = max over lines of max |K - x64| / S,
                          e(kernel) <= 2 e(oracle32) + 2^-23   (fp64: x SCALE); the 2 is the numpy model's, which
                          tests/test_partition_algebra.py runs on the chunkings and line lengths of this table
The slab entries run two ranks of a capi.LocalGroup on one card, the slabs' fields concatenated.

Largest e(kernel) / e(oracle32) measured on one MI355X (printed with -s: "RATIO ..."), over next and the merged temp;
e(oracle32) was 6.0e-8 .. 1.5e-6 (h = 0.004 .. 0.002 on every new grid: see launch_shape_cases._h):
    fp32 (16,8,32)                                   X 0.99   Y 1.23
    fp32 (16,16,32)                                  X 1.10   Y 1.03      late start (order 0x440)  Y 1.17
    fp32 (16,32,32), fused and unfused alike         X 1.08   Y 1.16
    fp32 order 0 on 32-line tiles (1024 workgroups)  X 1.02   Y 1.01
    fp64 (16,8,32), (16,16,16) (of the scaled e)     X 0.60   Y 0.57
    fp32 Z: 32 lanes 1.21; 64 lanes 1.60; 16 lanes with LG 2, 4, 8, 16: 1.00; 64 lanes with LG 2: 1.01; a pair of waves 1.18
    fp64 Z: 16 / 64 lanes, the pair, 32 lanes with LG 2 (of the scaled e) 0.59
    x-slabs on 2 ranks, five instances, both passes  X 1.32
    the bc_cases grids named in the table            as in tests/test_gpu_bc_matrix.py (X 1.52, Y 1.00, Z 1.63; fp64 0.52)
Three arithmetic-only mutations that only these entries reach (the back-substitution of the 32-chunk interface solve x (1 + 2^-18);
the W carried from row to row of a Z group x (1 + 2^-6); d' of the XB = 2 pass x 1.001 from the fourth chunk on) fail 8, 1 and 3
of these tests and none of tests/test_gpu_part.py's sweeps or tests/test_gpu_bc_matrix.py: DESIGN.md section 5.
"""
import numpy as np
import pytest

import bc_cases as BC
import launch_shape_cases as LS
from cmc_fluid_solver_amd import capi, grids
from cmc_fluid_solver_amd.slab import slab_range
from test_gpu_part import TOL_SWEEP, rel
from test_gpu_part_f64 import SCALE

pytestmark = pytest.mark.gpu

DT = BC.DT
LAYERS = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
RUNS = [(n, f) for n in LS.NAMES for f in LS.CASES[n].fuses]


def setup(s, c, fuse):
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_PART)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    if c.dtype == np.float64:
        s.set_option(capi.OPT_F64_PART, 1)


def seed(s, name, x=slice(None)):
    """the seeded state in cur and temp, the sentinel in next (planes x of the grid)"""
    cur, tmp = LS.seeded(name)
    s.upload_layer(capi.LAYER_CUR, [f[x] for f in cur]); s.upload_layer(capi.LAYER_TEMP, [f[x] for f in tmp])
    s.upload_layer(capi.LAYER_NEXT, [np.full(f[x].shape, BC.SENTINEL, s.dtype) for f in cur])


def two_sweeps(s, name, x=slice(None)):
    """The unmerged and the merged sweep of the entry's direction on context s: (next, temp) of the first, (next, temp) of the
    second; the launch is asserted after each."""
    c = LS.CASES[name]
    out = []
    for merge in (False, True):
        seed(s, name, x)
        s.sweep(c.d, DT, *LAYERS, merge=merge)
        k = s.last_sweep_kernels()["XYZ"[c.d]]
        assert k.split("+")[0] == "part" and (c.ranks == 1) == (k == "part"), k
        for pass_, want in ((0, c.record), (1, c.record1)):
            got = s.last_sweep_launch(c.d, pass_)
            assert got == LS.record_dict(want), "%s pass %d launched %s, the entry is there for %s" % (name, pass_, got, LS.record_dict(want))
        out += [s.download_layer(capi.LAYER_NEXT), s.download_layer(capi.LAYER_TEMP)]
    return out


def run(name, fuse):
    c = LS.CASES[name]
    g = LS.grid(name)
    params = capi.fluid_params(c.dtype, *BC.PARAMS)
    if c.ranks == 1:
        s = capi.Solver(g, params, c.dtype)
        setup(s, c, fuse)
        try:
            return two_sweeps(s, name)
        finally:
            s.close()

    def slab(r, sv):
        setup(sv, c, fuse)
        return two_sweeps(sv, name, slice(*slab_range(g.dimx, r, c.ranks)))
    grp = capi.LocalGroup(g, params, c.ranks, c.dtype)
    try:
        per_rank = grp.run(slab)
    finally:
        grp.close()
    return [[np.concatenate([r[k][v] for r in per_rank], axis=0) for v in range(4)] for k in range(4)]


@pytest.mark.parametrize("name,fuse", RUNS)
def test_launch_shape(built, name, fuse):
    c = LS.CASES[name]
    g = LS.grid(name)
    R32, R64 = LS.sweep_reference(name, np.float32), LS.sweep_reference(name, np.float64)
    scale = SCALE if c.dtype == np.float64 else 1.0
    ref = R64 if c.dtype == np.float64 else R32
    _, tmp0 = LS.seeded(name)
    fluid = g.type == grids.NODE_IN
    written = [x != BC.SENTINEL for x in R64[0]]
    A, T0, A2, T = run(name, fuse)
    what = "%s %s fuse %d" % (name, "XYZ"[c.d], fuse)
    for v in range(4):
        assert np.isfinite(A[v]).all(), "field %d has non-finite values" % v
        r = rel(A[v], ref[0][v])
        assert r <= TOL_SWEEP * scale, "next after sweep %d: field %d rel-L2 %.2e > %.1e" % (c.d, v, r, TOL_SWEEP * scale)
        assert np.array_equal(A[v] == BC.SENTINEL, ref[0][v] == BC.SENTINEL), "the set of written cells differs from the reference's"
        assert np.array_equal(A2[v] == BC.SENTINEL, ref[0][v] == BC.SENTINEL), "merged sweep: the set of written cells differs from the reference's"
        assert np.array_equal(T0[v], tmp0[v].astype(c.dtype)), "temp must be untouched by a sweep without merge"
        assert np.array_equal(T[v][~fluid], tmp0[v][~fluid].astype(c.dtype)), "cells that are not NODE_IN are left as they were"
    ratios = BC.check_lines(A, R32[0], R64[0], written, c.d, what + ": next", scale)
    ratios += BC.check_lines(A2, R32[0], R64[0], written, c.d, what + ": next (merged sweep)", scale)
    ratios += BC.check_lines(T, R32[1], R64[1], [fluid] * 4, c.d, what + ": merged temp", scale)
    print("RATIO launch-shape %s fuse %d: %s" % (name, fuse, {"XYZ"[c.d]: "%.2f" % max(ratios)}))
