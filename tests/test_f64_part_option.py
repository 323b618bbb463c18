"""CPU: the public face of FS3D_OPT_F64_PART (fp64 partition kernels, off by default) and the algebra of the chunking only
the fp64 Z kernel uses -- two cells per lane, the interface system by parallel cyclic reduction across up to 128 chunks
(csrc/kernels_part.hip: k_sweep_part_z<double, ...>) -- stated by the numpy twin (cmc_fluid_solver_amd/partition.py) against the
sequential Thomas solve of the oracle."""
import os
import re

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi
from cmc_fluid_solver_amd import partition as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_id_in_the_binding_and_the_header():
    assert capi.OPT_F64_PART == 6
    text = open(os.path.join(ROOT, "include", "fs3d.h")).read()
    m = re.search(r"\bFS3D_OPT_F64_PART\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 6
    ids = [int(v) for v in re.findall(r"\bFS3D_OPT_[A-Z0-9_]+\s*=\s*(\d+)", text)]
    assert len(ids) == len(set(ids)), "two options share an id"
    assert "FS3D_DEFAULT_F64_PART" in text


def _system(n, nlines, dtype, seed, nrhs=4):
    """rows shaped like the solver's (tests/test_partition_algebra.py): b = 3/dt + 2 vis, a/c = -vis -+ q, BC rows at the ends"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-130, 130, (n, nlines))
    a = (-q - 325.0).astype(dtype); c = (q - 325.0).astype(dtype); b = np.full((n, nlines), 680.0, dtype)
    a[0] = 0; b[0] = 1; c[0] = 0            # NOSLIP start row
    a[-1] = -1; b[-1] = 2; c[-1] = 0        # FREE end row
    d = rng.uniform(-5, 5, (n, nrhs, nlines)).astype(dtype)
    return a, b, c, d


def _thomas_ref(a, b, c, d):
    from oracle import oracle as O
    n, nrhs, nl = d.shape
    out = np.empty((n, nrhs, nl), np.float64)
    for l in range(nl):
        for r in range(nrhs):
            out[:, r, l] = O.tridiag(np.ascontiguousarray(a[:, l], np.float64), np.ascontiguousarray(b[:, l], np.float64),
                                     np.ascontiguousarray(c[:, l], np.float64), np.ascontiguousarray(d[:, r, l], np.float64))
    return out


@pytest.mark.parametrize("n", [256, 128, 64, 30, 8])
def test_two_cell_chunks_with_cyclic_reduction(built, n):
    """fp64, chunks of two cells, interface system by cyclic reduction: <= 2e-15 rel-L2 from the sequential recurrence on lines
    of up to 256 cells (the eps64 / eps32 scaling of the fp32 distances; ~6e-16 in this model at 256 cells)."""
    a, b, c, d = _system(n, 16, np.float64, seed=n)
    x = pt.solve(a, b, c, d, list(range(0, n + 1, 2)), "pcr")
    ref = _thomas_ref(a, b, c, d)
    err = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print("n = %d: 2-cell chunks + PCR vs Thomas, fp64 rel-L2 %.2e" % (n, err))
    assert err <= 2e-15, err
    res = b[:, None] * x - d                 # the solution satisfies the rows (independent of any reference solve)
    res[1:] += a[1:, None] * x[:-1]
    res[:-1] += c[:-1, None] * x[1:]
    assert np.abs(res).max() <= 1e-9


def test_a_single_leading_cell_is_swept_the_same_way_down_and_up():
    """What lets the kernel run ONE elimination step per lane: with one cell before the interface cell the down-sweep's
    (l', c', d') and the up-sweep's (a', u', e') are the same numbers."""
    a, b, c, d = _system(2, 7, np.float64, seed=11)
    co = pt.chunk_eliminate(a, b, c, d)
    r = 1 / b[0]
    assert np.array_equal(co["Vf"], a[0] * r) and np.array_equal(co["Wf"], c[0] * r) and np.array_equal(co["Gf"], d[0] * r[None])
    assert np.array_equal(co["A"], -a[1] * (a[0] * r)) and np.array_equal(co["Bp"], b[1] - a[1] * (c[0] * r))
