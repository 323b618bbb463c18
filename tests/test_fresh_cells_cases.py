"""CPU: the fresh-cell rule as its numpy twin states it (cmc_fluid_solver_amd/fresh_cells.py) on the cases the GPU tests hold the
kernels to -- convexity, the round counts of a wall slab, the identity, independence of the visiting order -- and the declarations
of the entries and of the option in include/fs3d.h and in capi.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import abi_decls  # noqa: E402
import fresh_cells_cases as FC  # noqa: E402
from cmc_fluid_solver_amd import capi, fresh_cells, grids  # noqa: E402

DTYPES = {"f32": np.float32, "f64": np.float64}
ALL = [(c, s, p) for c in FC.CASES for s in FC.SIZES for p in DTYPES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("case,size,prec", ALL)
def test_filled_values_lie_between_the_donors_and_nothing_else_changes(case, size, prec):
    a, b = FC.pair(case, size)
    before = FC.fields(size, DTYPES[prec], 11)
    after, info = FC.expected(case, size, DTYPES[prec], 11)
    donor, fresh = fresh_cells.classes(a.type, b.type)
    assert info[0] == int(fresh.sum()) and info[1] + info[3] == info[0] and 0 <= info[2] <= 250
    changed = np.zeros(donor.shape, bool)
    for x, y in zip(before, after):
        assert y.dtype == x.dtype
        diff = bits(x) != bits(y)
        assert not diff[~fresh].any()                    # donors and other cells: never written
        changed |= diff
        if donor.any() and diff.any():
            assert y[diff].min() >= x[donor].min() and y[diff].max() <= x[donor].max()
    assert int(changed.sum()) == info[1]                 # (seeded fields: a mean never equals what the cell held in all four)
    if case in FC.LEAVES_SOME:
        assert info[3] > 0
    elif case != "none":
        assert info[3] == 0 and info[0] > 0


@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("case", list(FC.ROUNDS))
def test_round_counts(case, size):
    assert FC.expected(case, size, np.float32, 11)[1][2] == FC.ROUNDS[case]


@pytest.mark.parametrize("t", [1, 2, 5, 6])
def test_a_wall_slab_fills_in_half_its_thickness_from_both_sides_and_in_all_of_it_from_one(t):
    for both in (True, False):
        a, b = grids.box(12, 6, 6), grids.box(12, 6, 6)
        lo = 2 if both else 1
        FC._wall(a, FC._slab(lo, lo + t - 1))
        seeded = [np.ascontiguousarray(f[:, :6, :6]) for f in FC.fields("12x10x16", np.float64, 3)]
        out, info = fresh_cells.fill_fresh_cells(a.type, b.type, seeded)
        assert info == (t * 16, t * 16, (t + 1) // 2 if both else t, 0), (t, both, info)


@pytest.mark.parametrize("size", list(FC.SIZES))
def test_none_is_the_identity(size):
    before = FC.fields(size, np.float32, 11)
    after, info = FC.expected("none", size, np.float32, 11)
    assert info == (0, 0, 0, 0)
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))


def test_capped_leaves_the_deeper_cells_untouched():
    a, b = FC.pair("capped", "12x10x16")
    before = FC.fields("12x10x16", np.float32, 11)
    after, info = FC.expected("capped", "12x10x16", np.float32, 11)
    assert info[2] == 2 and info[3] == 3 * 8 * 14        # the slab i = 1..5 fills from i = 6: planes 5 and 4 in two rounds
    for x, y in zip(before, after):
        assert np.array_equal(bits(x[1:4]), bits(y[1:4])) and not np.array_equal(bits(x[4:6, 1:-1, 1:-1]), bits(y[4:6, 1:-1, 1:-1]))


@pytest.mark.parametrize("case,size,prec", ALL)
def test_the_visiting_order_does_not_matter(case, size, prec):
    a, b = FC.pair(case, size)
    fresh = np.flatnonzero(fresh_cells.classes(a.type, b.type)[1])
    out, info = fresh_cells.fill_fresh_cells(a.type, b.type, FC.fields(size, DTYPES[prec], 11), FC.MAX_ROUNDS.get(case, 0), order=fresh[::-1])
    want, winfo = FC.expected(case, size, DTYPES[prec], 11)
    assert info == winfo
    for x, y in zip(out, want):
        assert np.array_equal(bits(x), bits(y))


def test_mixed_origin_has_fresh_cells_of_every_origin():
    a, b = FC.pair("mixed-origin", "9x7x11")
    fresh = fresh_cells.classes(a.type, b.type)[1]
    assert {grids.NODE_OUT, grids.NODE_BOUND, grids.NODE_VALVE} <= set(a.type[fresh].tolist())


def test_faces_has_fresh_cells_on_faces_edges_and_corners():
    for size, (nx, ny, nz) in FC.SIZES.items():
        a, b = FC.pair("faces", size)
        fresh = fresh_cells.classes(a.type, b.type)[1]
        assert fresh[0, 0, 0] and fresh[-1, -1, -1] and fresh[0, 0, 2] and fresh[0, 2, 0] and fresh[1, 0, 0]
        for face in (fresh[0, 4:6, 5:8], fresh[-1, 4:6, 5:8], fresh[4:7, 0, 5:8], fresh[4:7, -1, 5:8], fresh[4:7, 4:6, 0], fresh[4:7, 4:6, -1]):
            assert face.all()


def test_bad_arguments():
    a, b = FC.pair("none", "9x7x11")
    f = FC.fields("9x7x11", np.float32, 1)
    for bad in (-1, 251):
        with pytest.raises(ValueError):
            fresh_cells.fill_fresh_cells(a.type, b.type, f, bad)


# ---- the declarations ----------------------------------------------------------------------------------------------------------

ENTRIES = ("fs3d_fill_fresh_cells_dev", "fs3d_fill_fresh_cells", "fs3d_last_fill_device_ms")


def test_header_declares_the_entries_and_the_option_and_the_binding_lists_them():
    for name in ENTRIES:
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS, name
    assert abi_decls.enumerators()["FS3D_OPT_FRESH_CELLS"] == 9 and capi.OPT_FRESH_CELLS == 9
    assert len(capi.SYMBOLS["fs3d_fill_fresh_cells_dev"][1]) == 5 and len(capi.SYMBOLS["fs3d_fill_fresh_cells"][1]) == 4
    for method in ("fill_fresh_cells", "fill_fresh_cells_dev", "last_fill_device_ms"):
        assert callable(getattr(capi.Solver, method))


def test_library_exports_the_entries(built):
    import ctypes
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), name
