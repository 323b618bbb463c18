"""The cases behind tests/golden/output_record_digests.json: every filtered and derived result record the library writes -- whole
grid and x-slabs, host and device entries, `next` and a time statistic as the source -- pinned by the sha256 of its bytes.  Shared by
the recorder (tests/golden/make_output_record_digests.py), the GPU test (test_gpu_output_record_digests.py) and the CPU test of the
fields (test_output_digest_cases.py); building the cases and the fields needs no GPU.

The other GPU tests of the records hold the box means to the twin bit for bit on fields whose double sums are exact in any order, and
within a derived bound elsewhere: a change in the ORDER of a kernel's sums passes them all.  The fields here are made so that the
order shows: value = +-m * 2^e with m an odd 24-bit integer, from an integer hash of the cell index -- no libm, no float RNG, the
same bits on every machine.  e falls into one of two clusters of JITTER binades, GAP = 30 binades apart: a double sum of fp32 values
rounds only where its terms span more than 29 binades, and with the exponents spread evenly over 40 binades the small boxes of these
cases (a dozen fluid cells) mostly hold none that do -- on 23 x 13 x 11 -> 5 x 4 x 7 the reversed sum then differed in 38 of 120 boxes
and on 13 x 11 x 10 in 11 of 115, short of the third that test_output_digest_cases.py asks for.  fp64 adds a second such term 28
binades below the first, so that the value fills the mantissa (24 + 4 + 24 = 52 bits).  Every value is exact in the context's type
(asserted)."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import output_slabs_cases as OC  # noqa: E402
from test_gpu_output_filter import COARSE, GENERAL, GRIDS, MODES, PARAMS, make_nodes, set_mode  # noqa: E402
from cmc_fluid_solver_amd import grids  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "output_record_digests.json")
DTYPES = [np.float32, np.float64]
LONG_DIMS = (3, 3, 600)
# (dims, outdims) of the whole-grid records, and (dims, outdims, ranks) of the slab records
WHOLE = [(dims, od) for dims in GRIDS for od in (COARSE, (0, 0, 0))] + [(LONG_DIMS, (2, 2, 300)), (LONG_DIMS, (1, 1, 599))]
SLABS = list(OC.CASES)
DEV_WHOLE, DEV_SLABS = WHOLE[2], SLABS[1]                        # (23, 13, 11) -> (5, 4, 7): the whole grid, and 3 slabs
STAT_DIMS, STAT_OD, STAT_RANKS, STAT_STEPS, STAT_DT = (23, 13, 11), (5, 4, 7), 3, 4, 0.05
GAP, JITTER = 30, 2


def _mix(x):
    """splitmix64's finaliser on a uint64 array (the products wrap)"""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hashed_fields(shape, dtype, salt):
    """Four order-sensitive fields of the module docstring; field v of cell c hashes 4 * c + v + salt * 2^40"""
    n = int(np.prod(shape))
    out = []
    for v in range(4):
        h = _mix(np.arange(n, dtype=np.uint64) * np.uint64(4) + np.uint64(v) + (np.uint64(salt) << np.uint64(40)))
        mant = ((h & np.uint64(0x7FFFFF)) | np.uint64(0x800001)).astype(np.int64)          # odd, 24 bits
        sign = 1 - 2 * ((h >> np.uint64(24)) & np.uint64(1)).astype(np.int64)
        pick = h >> np.uint64(25)                                   # bit 0: the cluster, the bits above: the place in it
        exp = (pick & np.uint64(1)).astype(np.int64) * GAP + ((pick >> np.uint64(1)) % np.uint64(JITTER)).astype(np.int64) - (GAP + JITTER) // 2 - 23
        val = np.ldexp((sign * mant).astype(np.float64), exp)
        if np.dtype(dtype) == np.float64:
            low = (((h >> np.uint64(32)) & np.uint64(0x7FFFFF)) | np.uint64(0x800001)).astype(np.int64)
            val = val + np.ldexp((sign * low).astype(np.float64), exp - 28)
            assert np.array_equal(np.ldexp(val, -(exp - 28)), (sign * ((mant << 28) + low)).astype(np.float64)), "52 bits: exact in fp64"
        f = val.astype(dtype)
        assert np.array_equal(f.astype(np.float64), val), "every value is exact in the context's type"
        out.append(f.reshape(shape))
    return out


def nodes_of(dims):
    """make_nodes of the filter tests; the long thin grid is the one of their long-line test (its one fluid line, a NODE_OUT run on it)"""
    if dims != LONG_DIMS:
        return make_nodes(dims, GENERAL)
    n = grids.box(*dims)
    n.dx, n.dy, n.dz = GENERAL
    n.type[1, 1, 250:262] = grids.NODE_OUT
    return n


def name(dtype):
    return np.dtype(dtype).name


def digest(V, T):
    return hashlib.sha256(np.ascontiguousarray(V).tobytes() + np.ascontiguousarray(T).tobytes()).hexdigest()


def whole_id(dims, od):
    return "whole-%s-to-%s" % ("x".join(map(str, dims)), "x".join(map(str, od)))


def slab_id(case):
    return "slabs-" + OC.case_id(case)


def mode_key(base, dtype, filter, vector, entry="host"):
    return "%s-%s-filter%d-vector%d-%s" % (base, name(dtype), filter, vector, entry)


# ---- the runs (GPU): each returns {digest id: sha256} -------------------------------------------------------------------------------

def _dev_arrays(od, dtype):
    import torch
    td = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
    dV = torch.full(tuple(od) + (3,), float("nan"), dtype=td, device="cuda")
    dT = torch.full(tuple(od), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return dV, dT


def run_whole(dims, od, dtype, dev=False):
    from cmc_fluid_solver_amd import capi
    s = capi.Solver(nodes_of(dims), capi.fluid_params(dtype, *PARAMS), dtype)
    s.upload_layer(capi.LAYER_NEXT, hashed_fields(dims, dtype, 1))
    full = tuple(o or d for o, d in zip(od, dims))
    out = {}
    for filter, vector in MODES:
        set_mode(s, filter, vector)
        out[mode_key(whole_id(dims, od), dtype, filter, vector)] = digest(*s.GetLayer(od))
        if dev:
            dV, dT = _dev_arrays(full, dtype)
            assert s.GetLayerDev(dV, dT, od) == (0, full[0])
            s.synchronize()
            out[mode_key(whole_id(dims, od), dtype, filter, vector, "dev")] = digest(dV.cpu().numpy(), dT.cpu().numpy())
    s.close()
    return out


def run_slabs(case, dtype, dev=False):
    from test_gpu_output_slabs import group, record
    from cmc_fluid_solver_amd.slab import out_rows
    dims, od, nranks = case
    grp = group(nodes_of(dims), nranks, dtype, hashed_fields(dims, dtype, 2))
    full = tuple(o or d for o, d in zip(od, dims))
    out = {}
    for filter, vector in MODES:
        out[mode_key(slab_id(case), dtype, filter, vector)] = digest(*record(grp, od, filter, vector))
        if dev:
            dV, dT = _dev_arrays(full, dtype)

            def work(rank, s):
                rows = s.GetLayerDev(dV, dT, od)
                s.synchronize()
                return rows
            assert grp.run(work) == [out_rows(s.x0, s.x1, dims[0], full[0]) for s in grp.solvers]
            out[mode_key(slab_id(case), dtype, filter, vector, "dev")] = digest(dV.cpu().numpy(), dT.cpu().numpy())
    grp.close()
    return out


def run_stats(dtype):
    """Source 2 with moment 1 (the Reynolds stresses) after four steps on the bit-exact kernels (FS3D_DEFAULT_KERNEL = 4 in the
    environment when the contexts are made), through the box mean: the whole grid and 3 slabs"""
    from test_gpu_output_slabs import group, record
    from cmc_fluid_solver_amd import capi
    assert os.environ.get("FS3D_DEFAULT_KERNEL") == "4"
    nodes = grids.box_with_obstacle(*STAT_DIMS)
    base = [np.ascontiguousarray(a, dtype) for a in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    start = grids.perturb(base, seed=8)

    def steps(rank, s):
        s.set_option(capi.OPT_TIME_STATS, 2)
        s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
        s.upload_layer(capi.LAYER_CUR, [f[s.x0:s.x1] for f in start])
        for _ in range(STAT_STEPS):
            s.UpdateBoundaries()
            s.TimeStep(STAT_DT, 2, 1, True)

    def select(s):
        s.set_option(capi.OPT_OUTPUT_SOURCE, 2)
        s.set_option(capi.OPT_OUTPUT_MOMENT, 1)
    one = capi.Solver(nodes, capi.fluid_params(dtype, *PARAMS), dtype)
    steps(0, one)
    select(one)
    set_mode(one, 1, 0)
    out = {"stats-whole-%s" % name(dtype): digest(*one.GetLayer(STAT_OD))}
    one.close()
    grp = group(nodes, STAT_RANKS, dtype)
    grp.run(steps)
    out["stats-slabs-on-%d-%s" % (STAT_RANKS, name(dtype))] = digest(*record(grp, STAT_OD, 1, 0, before=select))
    grp.close()
    return out


# every run of the file: (pytest id, function, arguments)
RUNS = [("%s-%s" % (whole_id(*c), name(t)), run_whole, c + (t, c == DEV_WHOLE)) for c in WHOLE for t in DTYPES] + \
       [("%s-%s" % (slab_id(c), name(t)), run_slabs, (c, t, c == DEV_SLABS)) for c in SLABS for t in DTYPES] + \
       [("stats-%s" % name(t), run_stats, (t,)) for t in DTYPES]
