"""No GPU: the numpy statement of the filtered and derived result records on x-slabs (layer_output.straddling_rows, slab_partials,
finish_slabs; FS3D_OPT_OUTPUT_SLABS) against layer_output of the GLOBAL grid, on the cases the GPU test runs
(output_slabs_cases.py) -- and the proof that those cases can fail: slabs that do not talk write another record."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import output_slabs_cases as OC  # noqa: E402
from test_gpu_output_filter import assert_within_bound, exact_fields, general_fields, make_nodes  # noqa: E402
from cmc_fluid_solver_amd import layer_output as LO  # noqa: E402

DTYPES = [np.float32, np.float64]
IDS = [OC.case_id(c) for c in OC.CASES]


def slab_record(type, fields, cuts, outdims, filter, vector, spacing):
    per_rank = [LO.slab_partials(type, fields, cuts, r, outdims, filter, vector, spacing) for r in range(len(cuts))]
    return LO.finish_slabs(type, fields, cuts, per_rank, outdims, vector, spacing), per_rank


@pytest.mark.parametrize("case,want", list(zip(OC.CASES, OC.STRADDLING)), ids=IDS)
def test_straddling_rows(case, want):
    dims, od, nranks = case
    cuts = OC.cuts_of(dims[0], nranks)
    assert cuts[0][0] == 0 and cuts[-1][1] == dims[0] and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    rows = LO.straddling_rows(cuts, dims[0], od[0])
    assert rows == want and len(rows) <= nranks - 1
    owned = [LO.owned_rows(cuts, r, dims[0], od[0]) for r in range(nranks)]
    assert owned[0][0] == 0 and owned[-1][1] == (od[0] or dims[0]) and all(a[1] == b[0] for a, b in zip(owned, owned[1:]))


def test_the_slabs_a_straddling_row_lies_on():
    """13 -> 2 on 4 slabs [0,4) [4,7) [7,10) [10,13): row 0 = [0,6) on the ranks 0 and 1, row 1 = [6,13) on 1, 2 and 3; the ranks
    2 and 3 own no row and still hold partials.  6 -> 1 on 3 slabs: the one row on all of them."""
    for (dims, od, nranks), on in ((OC.CASES[3], {0: [0, 1], 1: [1, 2, 3]}), (OC.CASES[6], {0: [0, 1, 2]})):
        nodes = make_nodes(dims, OC.POW2)
        nodes.type[:, 1:-1, 1:3] = LO.NODE_IN                    # every plane holds fluid in some box
        fields = exact_fields(dims, np.float32, 3)
        cuts = OC.cuts_of(dims[0], nranks)
        if nranks == 4:
            assert cuts == [(0, 4), (4, 7), (7, 10), (10, 13)]
            assert [LO.owned_rows(cuts, r, 13, 2) for r in range(4)] == [(0, 1), (1, 2), (2, 2), (2, 2)]
        parts = [LO.slab_partials(nodes.type, fields, cuts, r, od, 1, 0)[3] for r in range(nranks)]
        for row, ranks in on.items():
            assert [r for r in range(nranks) if parts[r][row][4].any()] == ranks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", OC.CASES, ids=IDS)
def test_exact_fields_equal_the_global_record_bit_for_bit(case, dtype):
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.POW2)
    fields = exact_fields(dims, dtype, 21)
    cuts = OC.cuts_of(dims[0], nranks)
    for filter, vector in OC.MODES:
        (V, T), per_rank = slab_record(nodes.type, fields, cuts, od, filter, vector, OC.POW2)
        eV, eT = LO.layer_output(nodes.type, fields, od, filter, vector, OC.POW2)
        assert V.dtype == eV.dtype and np.array_equal(V, eV) and np.array_equal(T, eT), (filter, vector)
        assert sorted(per_rank[0][3]) == (LO.straddling_rows(cuts, dims[0], od[0]) if filter else [])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", OC.CASES, ids=IDS)
def test_general_fields_stay_within_the_derived_bound(case, dtype):
    """The bound of test_gpu_output_filter.py: the rule leaves the order of the double sum free, so a sum split at the cuts is one
    of the orders it covers.  The point vorticity is a gather: bit for bit, on general spacings too."""
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.GENERAL)
    fields = general_fields(dims, dtype, 22)
    cuts = OC.cuts_of(dims[0], nranks)
    for filter, vector in OC.MODES:
        (V, T), _ = slab_record(nodes.type, fields, cuts, od, filter, vector, OC.GENERAL)
        if filter:
            assert_within_bound(nodes.type, fields, od, vector, OC.GENERAL, V, T, "%s %s vector %d" % (OC.case_id(case), np.dtype(dtype).name, vector))
        else:
            eV, eT = LO.layer_output(nodes.type, fields, od, 0, 1, OC.GENERAL)
            assert np.array_equal(V, eV) and np.array_equal(T, eT)


@pytest.mark.parametrize("case,strad", list(zip(OC.CASES, OC.STRADDLING)), ids=IDS)
def test_the_cases_can_fail(case, strad):
    """Slabs that exchange nothing -- boxes clipped at the cuts, no curl on a cut's planes -- write another record than the global
    one, in a row at a cut and nowhere else: with a straddling row the box mean of the velocity differs there, and without one the
    point vorticity differs on the planes beside the cuts."""
    dims, od, nranks = case
    nodes = make_nodes(dims, OC.POW2)
    fields = exact_fields(dims, np.float32, 21)
    cuts = OC.cuts_of(dims[0], nranks)
    at_cuts = OC.rows_at_cuts(cuts, dims[0], od[0])
    differing = {}
    for filter, vector in OC.MODES:
        nV, nT = OC.naive_record(nodes.type, fields, cuts, od, filter, vector, OC.POW2)
        eV, eT = LO.layer_output(nodes.type, fields, od, filter, vector, OC.POW2)
        assert not np.isnan(nV).any() and not np.isnan(nT).any()
        rows = sorted(set(np.nonzero((nV != eV).any(axis=(1, 2, 3)) | (nT != eT).any(axis=(1, 2)))[0].tolist()))
        assert set(rows) <= set(at_cuts), (filter, vector, rows, at_cuts)
        differing[(filter, vector)] = rows
    print(OC.case_id(case), "rows at the cuts", at_cuts, "rows the naive record gets wrong", differing)
    if strad:
        assert differing[(1, 0)] == strad and set(strad) <= set(differing[(1, 1)])
    else:
        assert differing[(0, 1)], "the curl on the planes beside a cut"
