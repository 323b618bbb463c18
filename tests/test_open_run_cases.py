"""CPU conditions of the open-run grids of tests/open_run_cases.py: what tests/test_gpu_open_runs.py takes for granted before it
blames a kernel.  Every grid goes through the host table builder (tests/geom_tables_test.cpp, with the sanitizers) and equals the
numpy restatement; it has the oracle's segment counts, no shared FREE cell, and the stale / NODE_IN START properties its entry
states; the CPU oracle walks three steps on the seeded state in both precisions; and on every case flagged stale-sensitive the
oracle's result really depends on the first contents of half and next alone -- a case that loses this stops testing the stale
read, and this is where it shows."""
import numpy as np
import pytest

import open_run_cases as OC
import test_geom_tables as GT
from cmc_fluid_solver_amd import capi, grids
from geom_rules import ROW_END, ROW_INTERIOR, ROW_SKIP, ROW_START
from test_geom_tables import program  # noqa: F401  (the fixture that builds the host program)


@pytest.mark.parametrize("name", OC.EVERY)
def test_tables_and_stated_properties(built, program, tmp_path, name):  # noqa: F811
    g, c = OC.grid(name), OC.CASES[name]
    t = GT.check_single(program, tmp_path, g)                # builder == restatement, nseg == the oracle's
    assert t["shared_free"] is False
    assert (t["stale_in_cells"] > 0) == c.stale, t["stale_in_cells"]
    assert t["stale_in_cells"] == sum(int(OC.stale_mask(name, d).sum()) for d in range(3))
    assert OC.in_start_count(name) == c.in_starts
    print("%s: stale_in_cells %d, NODE_IN START cells %d, segments %s" % (name, t["stale_in_cells"], c.in_starts, t["nseg"]))
    # the closed twin has neither property
    tw = GT.restate(OC.grid(name, closed=True))
    assert tw["stale_in_cells"] == 0 and tw["shared_free"] is False


@pytest.mark.parametrize("name", OC.EVERY)
def test_no_row_reads_outside_the_arrays(built, name):
    """An interior row reads its six neighbours by flat index (id +- plane, +- dimz, +- 1): inside the arrays iff the cell lies in
    the planes 1 .. dimx - 2.  The reference has no check of its own, so a NODE_IN cell of plane 0 or dimx - 1 on a Y or Z
    segment has no defined answer; the windows in those planes are corner windows for this reason."""
    for d, kind in enumerate(OC.kinds(name)):
        rows = np.argwhere(kind == ROW_INTERIOR)
        assert rows[:, 0].min() >= 1 and rows[:, 0].max() <= OC.grid(name).dimx - 2, "XYZ"[d]


def test_what_the_constructions_are_for(built):
    """The cells each construction is named after are where it says."""
    kx = OC.kinds("x_obstacle_then_open")[0][:, 12, 15]      # a line through the block: segment, END, OUT, START .. stale tail
    assert kx[0] == ROW_START and kx[11] == ROW_END and kx[16] == ROW_SKIP and (kx[17:] == ROW_SKIP).all()
    assert (OC.grid("x_obstacle_then_open").type[17:, 12, 15] == grids.NODE_IN).all()
    kx = OC.kinds("x_through")[0][:, 6, 8]
    assert (kx == ROW_SKIP).all() and (OC.grid("x_through").type[:, 6, 8] == grids.NODE_IN).all()
    kx = OC.kinds("x_lone_cell")[0][:, 6, 8]
    assert kx[0] == ROW_SKIP and kx[1] == ROW_START and OC.stale_mask("x_lone_cell", 0)[0].sum() == OC.window_mask("x_lone_cell").sum()
    assert not OC.stale_mask("x_lone_cell", 0)[1:].any()
    kx = OC.kinds("x_lo")[0][:, 6, 8]
    assert kx[0] == ROW_START and kx[1] == ROW_INTERIOR and OC.grid("x_lo").type[0, 6, 8] == grids.NODE_IN
    # the windows in the j and k faces are stale in their own direction only; those in the i faces in all three, and beyond the
    # window plane in X only
    for d, name in ((1, "y_hi"), (2, "z_hi")):
        assert [bool(OC.stale_mask(name, e).any()) for e in range(3)] == [e == d for e in range(3)]
    w = OC.window_mask("x_hi")
    assert all((OC.stale_mask("x_hi", d) & w).sum() == w.sum() for d in range(3))
    assert OC.stale_mask("x_hi", 0)[1:-1].any() and not OC.stale_mask("x_hi", 1)[:-1].any() and not OC.stale_mask("x_hi", 2)[:-1].any()
    # all_three: stale cells of every direction inside the shell, Z-stale cells that X segments write, NODE_IN Z STARTs
    inner = np.zeros(OC.grid("all_three").shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert all((OC.stale_mask("all_three", d) & inner).any() for d in range(3)) and OC.in_start_count("all_three") == 20
    assert (OC.stale_mask("all_three", 2) & (OC.kinds("all_three")[0] != ROW_SKIP)).any()


def test_partition_shapes(built):
    """The group k 32..63 of rows 10..38: one uniform column whose NODE_IN cells are all stale (part_*_group), not uniform with
    k 32 left closed (part_*_cut); stale and solved Z lines side by side (part_z_mixed); dimz a multiple of 4 wherever the
    partition kernels are asked."""
    for d, axis in ((0, "x"), (1, "y")):
        t = GT.restate(OC.grid("part_%s_group" % axis))
        b0, _, ids = GT.flag_bits(t, d, 68)
        col = t["ucol%d" % d].reshape(-1, GT.UCOL_PITCH)[ids[11, 1]]
        n = 70 if d == 0 else 40
        kind, ty = (col[:n] >> (4 * d)) & 3, (col[:n] >> GT.CODE_TYPE_SHIFT) & 3
        assert b0[11, 1] == 1 and (kind == ROW_SKIP).all() and (ty[1:] == grids.NODE_IN).all()
        b0, _, _ = GT.flag_bits(GT.restate(OC.grid("part_%s_cut" % axis)), d, 68)
        assert b0[11, 1] == 0 and b0[11, 0] == 1
    st = OC.stale_mask("part_z_mixed", 2).any(axis=2)        # [i][j]: stale Z lines
    assert st[11, 9:21].all() and not st[11, :9].any() and not st[11, 21:].any() and not st[9].any()
    for name in OC.PART:
        assert (OC.grid(name).dimz % 4 == 0) == ("Z" in OC.CASES[name].part or name.startswith("part_"))
    assert OC.grid("line_fallback").dimz % 4 != 0 and OC.CASES["line_fallback"].part == ""
    # z_hi_lone_lane: cell dimz - 1 is alone in the last X/Y tile (32 lines in fp32, 16 in fp64) and is an X and a Y row
    g = OC.grid("z_hi_lone_lane")
    assert g.dimz % 32 == 1 and g.dimz % 16 == 1
    assert all((OC.kinds("z_hi_lone_lane")[d][6:11, 5:9, -1] == ROW_INTERIOR).all() for d in (0, 1))
    # part_y_row_behind: in fp64 the Z kernel holds a 68-cell line in one wave-wide access (2 cells per lane: 65 .. 128 cells), and
    # part_launch_z groups its rows by LG = 16 halved while ceil(dimy / LG) dimx < 4096: 2 here, so line dimy - 1 = 92 opens a group
    g = OC.grid("part_y_row_behind")
    LG = 16
    while LG > 1 and -(-g.dimy // LG) * g.dimx < 4096:
        LG //= 2
    assert 64 < g.dimz <= 128 and LG == 2 and (g.dimy - 1) % LG == 0
    assert (OC.kinds("part_y_row_behind")[2][10:14, -1, 32:64] == ROW_INTERIOR).all()
    # part_z_row_behind_132: in fp32 the Z kernel holds a 132-cell line in one wave-wide access (4 cells per lane: 129 .. 256 cells, 33
    # lanes in use), one row per group on so small a grid; in fp64 a pair of waves holds it.  The window reaches into lane 32.
    g = OC.grid("part_z_row_behind_132")
    assert 128 < g.dimz <= 256 and g.dimz % 4 == 0 and g.dimy * g.dimx < 4096
    assert (OC.kinds("part_z_row_behind_132")[2][4:8, -1, 100:131] == ROW_INTERIOR).all()
    assert OC.stale_mask("part_z_row_behind_132", 1)[4:8, -1, 100:131].all() and not OC.stale_mask("part_z_row_behind_132", 2).any()


@pytest.mark.parametrize("name", OC.EVERY)
def test_oracle_walks_three_steps(built, name):
    for dtype in (np.float32, np.float64):
        for n, st in enumerate(OC.steps_reference(name, dtype, get_layers=True)):
            assert st.rc == 0 and st.err < 0.01, (n, st.rc, st.err)
            for f in st.cur + st.next + st.temp:
                assert np.isfinite(f).all()
            print("%s %s step %d: diffError %.3e" % (name, np.dtype(dtype).name, n, st.err))


@pytest.mark.parametrize("name", OC.EVERY)
def test_stale_sensitivity_is_as_stated(built, name):
    """Other contents in half and next only: cur after the first and after the third step differs on a sensitive case, and is
    the same bit for bit on the others (what they read was written earlier in the same step)."""
    a, b = OC.steps_reference(name, np.float32), OC.steps_reference(name, np.float32, alt=True)
    for step in (0, 2):
        differing = [int((x != y).sum()) for x, y in zip(a[step].cur, b[step].cur)]
        print("%s step %d: cells of cur that change with the stale contents, per field: %s" % (name, step, differing))
        assert all(n > 0 for n in differing) == OC.CASES[name].sensitive, (step, differing)
        assert any(n > 0 for n in differing) == OC.CASES[name].sensitive, (step, differing)


@pytest.mark.parametrize("name", OC.PART)
def test_sentinel_sweeps_write_the_segment_cells(built, name):
    """One merged sweep with the sentinel in next: the oracle writes exactly the cells the tables put on a segment, and the
    merged temp of a stale cell is (temp + sentinel) / 2 of the uploaded values."""
    ref = OC.sentinel_sweep_reference(name, np.float32)
    tmp0 = OC.seeded(name)[capi.LAYER_TEMP]
    for d in range(3):
        on_seg = OC.kinds(name)[d] != ROW_SKIP
        stale = OC.stale_mask(name, d)
        for v in range(4):
            assert np.array_equal(ref[d][0][v] != OC.SENTINEL, on_seg)
            assert np.array_equal(ref[d][1][v][stale], (tmp0[v][stale] + np.float32(OC.SENTINEL)) * np.float32(0.5))
