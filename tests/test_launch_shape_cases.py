"""CPU conditions of the launch-shape table of tests/launch_shape_cases.py: what tests/test_gpu_launch_shapes.py takes for granted
before it blames a kernel.  Every template instance the dispatch of csrc/kernels_part.hip can reach has an entry, and so has every
way a launch parameter is computed; the grids are small; the END | START pair of every new grid sits on the two sides of the edge
the entry names, on a line whose two end rows are FREE; and the fp32 oracle really differs from the fp64 oracle on every field (the
per-line criterion divides by that distance)."""
import numpy as np
import pytest

import bc_cases as BC
import launch_shape_cases as LS
import test_geom_tables as GT
from cmc_fluid_solver_amd import grids
from geom_rules import ROW_END, ROW_INTERIOR, ROW_START

# Every instance the dispatch can reach, written out from the code: (precision, "xy", DIR, M, NCH, LT, XB) / (precision, "z", LPL, NW).
# Not here: the 16- and 64-line Y tiles and the 16-line X tiles of FS3D_PART_VARIANT, which only that environment variable
# reaches (tests/test_gpu_part.py holds them to the bits of the default instance).
INSTANCES = set()
for _dir in (0, 1):
    INSTANCES |= {("float32", "xy", _dir, 16, 4, 32, 0),      # part_dispatch_xy, float: n <= 64
                  ("float32", "xy", _dir, 16, 8, 32, 0),      # n <= 128
                  ("float32", "xy", _dir, 16, 16, 32, 0),     # n <= 256, the last return (Y always; X on small planes)
                  ("float32", "xy", _dir, 16, 32, 32, 0),     # n <= 512
                  ("float64", "xy", _dir, 16, 4, 32, 0),      # part_dispatch_xy, double: n <= 64
                  ("float64", "xy", _dir, 16, 8, 32, 0),      # n <= 128
                  ("float64", "xy", _dir, 16, 16, 16, 0)}     # n <= 256
INSTANCES.add(("float32", "xy", 0, 16, 16, 64, 0))            # n <= 256, DIR == 0 && dimy * ceil(dimz / 64) >= 512
for _xb in (1, 2):                                            # part_dispatch_xslab: XB 1 from carry_in && xcarry_in, XB 2 from xiface_pass
    INSTANCES |= {("float32", "xy", 0, 8, 4, 64, _xb),        # n <= 32 (XB 2: n % 8 == 0)
                  ("float32", "xy", 0, 16, 4, 32, _xb),       # n <= 64, not wide (XB 2: n % 16 == 0 from here on)
                  ("float32", "xy", 0, 16, 4, 64, _xb),       # n <= 64, wide
                  ("float32", "xy", 0, 16, 8, 32, _xb),       # n <= 128, not wide
                  ("float32", "xy", 0, 16, 8, 64, _xb),       # n <= 128, wide
                  ("float32", "xy", 0, 16, 16, 64, _xb)}      # n <= 256
for _p in ("float32", "float64"):                             # part_dispatch_z, C = 16 / sizeof(R) cells per lane
    INSTANCES |= {(_p, "z", 16, 1), (_p, "z", 32, 1), (_p, "z", 64, 1),      # n <= 16 C, 32 C, 64 C
                  (_p, "z", 64, 2)}                                           # n <= 128 C: a pair of waves per line


def test_every_dispatched_instance_has_an_entry():
    have = {k for c in LS.CASES.values() for k in LS.instance(c)}
    assert INSTANCES - have == set(), "no entry"
    assert have - INSTANCES == set(), "an entry names an instance the dispatch cannot reach"
    assert len(INSTANCES) == 35


def test_every_way_a_launch_parameter_is_computed_has_an_entry():
    xy = [r for c in LS.CASES.values() for r in (c.record, c.record1) if r and r[0] == 1]
    z = {np.dtype(c.dtype).name: [] for c in LS.CASES.values()}
    for c in LS.CASES.values():
        if c.record[0] == 2:
            z[np.dtype(c.dtype).name].append(c.record)
    # part_launch_xy: lane tiles fastest (1), rows fastest on 32-line tiles (0 from 1024 workgroups on), the late start, 64-line tiles
    assert {(r[3] <= 32, r[5]) for r in xy} == {(True, 1), (True, 0), (True, 0x440), (False, 0)}
    assert all((r[6] >= 1024) == (r[5] != 1) for r in xy if r[3] <= 32 and r[2] != 32)
    assert all(r[5] == 1 for r in xy if r[2] == 32)                                  # 512-cell lines: always lane tiles fastest
    # part_launch_z: every LG of the halving loop; in fp64 two rows in flight
    assert {r[3] for r in z["float32"]} == {1, 2, 4, 8, 16} and {r[3] for r in z["float64"]} == {1, 2}
    assert {(r[1], r[3]) for r in z["float32"]} >= {(16, 2), (64, 2)}                # several lines per access, and one
    # a pair of waves: an even and an odd number of tasks (odd: the last workgroup's second pair is past the end)
    assert {(c.record[4] * c.dims[0]) % 2 for c in LS.CASES.values() if c.record[0] == 2 and c.record[2] == 2} == {0, 1}
    # the unfused merge too on the 32-chunk instance, which no other grid of the suite below 512^3 reaches
    assert all((c.fuses == (0, 1)) == (c.record[0] == 1 and c.record[2] == 32) for c in LS.CASES.values())


@pytest.mark.parametrize("name", LS.NAMES)
def test_grid_is_small_and_the_record_fits_it(name):
    c = LS.CASES[name]
    assert max(c.dims) <= LS.MAX_DIM and int(np.prod(c.dims)) <= LS.MAX_CELLS
    assert c.dims[0] % c.ranks == 0 and (c.ranks == 1 or c.d == 0) and (c.record1 is None) == (c.ranks == 1)
    nx = c.dims[0] // c.ranks
    cells = 16 // np.dtype(c.dtype).itemsize
    for r in (c.record, c.record1):
        if r is None:
            continue
        assert (r[0] == 2) == (c.d == 2)
        if r[0] == 1:                              # M x NCH cells hold the line (the next smaller instance would not); one workgroup per row / plane and tile
            n = nx if c.d == 0 else c.dims[1]
            assert r[1] * r[2] // 2 < n <= r[1] * r[2] or (r[2] == 4 and n <= r[1] * r[2])
            assert r[6] == (c.dims[1] if c.d == 0 else nx) * -(-c.dims[2] // r[3])
        else:                                      # LPL x NW lanes of `cells` hold the line; rows of 64 / LPL lines in groups of LG
            assert c.dims[2] % cells == 0 and r[1] * r[2] * cells // 2 < c.dims[2] <= r[1] * r[2] * cells or (r[1] == 16 and c.dims[2] <= 16 * cells)
            rows = -(-c.dims[1] // (64 // r[1]))
            assert r[4] == -(-rows // r[3]) and r[5] == -(-r[4] * nx // (2 if r[2] == 2 else 4))


@pytest.mark.parametrize("name", [n for n in LS.NAMES if LS.CASES[n].grid is None])
def test_plate_rows_sit_on_both_sides_of_the_named_edge(built, name):
    """Some line of the sweep direction has the plate's END row (FREE, FREE) on the last cell of a unit and its START row on the
    first cell of the next, fluid on both sides, and FREE rows on the line's first and last cell."""
    c = LS.CASES[name]
    g = LS.grid(name)
    t = GT.restate(g)
    assert t["shared_free"] is False and t["stale_in_cells"] == 0
    assert t["nseg"] == GT.oracle_nseg(g)
    e = c.pos[c.d]
    assert (e + 1) % c.unit == 0
    if c.ranks > 1:
        assert c.unit == c.dims[0] // c.ranks
    L = np.moveaxis((t["code"].reshape(g.shape) >> (4 * c.d)) & 0xF, c.d, -1)
    free = GT.ROW_VELFREE | GT.ROW_TEMPFREE
    hit = (L[..., e] == ROW_END | free) & (L[..., e + 1] == ROW_START | free) & (L[..., e - 1] == ROW_INTERIOR) & (L[..., e + 2] == ROW_INTERIOR)
    ends = ((L[..., 0] & 3) == ROW_START) & ((L[..., 0] & free) != 0) & ((L[..., -1] & 3) == ROW_END) & ((L[..., -1] & free) != 0)
    print("%s: %d lines with END | START on cells %d | %d, %d of them between FREE end rows (%s .. %s)" % (
        name, hit.sum(), e, e + 1, (hit & ends).sum(), BC.code_name(L[..., 0].max()), BC.code_name(L[..., -1].max())))
    assert (hit & ends).any()
    # the whole open part of both faces of the direction couples: every line that starts on cell 0 starts and ends FREE
    starts = (L[..., 0] & 3) == ROW_START
    assert starts.any() and (ends | ~starts).all()


@pytest.mark.parametrize("name", LS.NAMES)
def test_the_fp32_oracle_differs_from_the_fp64_oracle_on_every_field(built, name):
    c = LS.CASES[name]
    g = LS.grid(name)
    R32, R64 = LS.sweep_reference(name, np.float32), LS.sweep_reference(name, np.float64)
    fluid = g.type == grids.NODE_IN
    for which, mask in ((0, None), (1, fluid)):
        for v in range(4):
            a, b = R32[which][v], R64[which][v]
            assert np.isfinite(a).all() and np.isfinite(b).all()
            written = b != BC.SENTINEL if mask is None else mask
            if mask is None:
                assert np.array_equal(a != BC.SENTINEL, written), "both precisions write the same cells"
            assert written.any() and np.abs(b[written]).max() > 0
            eo, _ = BC.line_error(a, b, written, c.d)
            print("%s %s field %d: e(oracle32) %.2e" % (name, ("next", "merged temp")[which], v, eo))
            assert eo > 0
