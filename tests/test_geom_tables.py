"""The host definition of the geometry tables (cmc_fluid_solver_amd/csrc/fs3d_tables.h: build_geom_tables), run on a CPU.

tests/geom_tables_test.cpp is built once with the address and undefined-behaviour sanitizers and run as a program of its own on
each case; any table that differs from the numpy restatement below, and any sanitizer report (a non-zero exit), fails the test.
The restatement uses whole-array operations on the node arrays and states each table as a property, not as the C++ loops.

The pair rule of the shared columns as the code has it: bit 1 lives on the even group g of a pair, and only an all-dead EVEN group
takes its partner's column (a 64-line tile reads the column of g); an all-dead odd group keeps its zero column.
"""
import os
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids
from geom_rules import ROW_END, ROW_SKIP, ROW_START, rule_kinds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UCOL_PITCH, CODE_TYPE_SHIFT, ROW_VELFREE, ROW_TEMPFREE = 512, 12, 4, 8


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geom_tables") / "geom_tables_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "geom_tables_test.cpp"), "-o", exe])
    return exe


def run_builder(program, tmp_path, g, x0=0, nx=None):
    """The C++ tables of the planes [x0, x0 + nx) of g, as a dict."""
    nx = g.dimx if nx is None else nx
    src, dst = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    with open(src, "wb") as f:
        np.array([g.dimx, g.dimy, g.dimz, x0, nx], np.int32).tofile(f)
        for a in (g.type, g.bc_vel, g.bc_temp):
            np.ascontiguousarray(a, np.uint8).tofile(f)
    r = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    head = np.frombuffer(raw, np.int64, 20)
    t = {"nseg": [int(v) for v in head[0:3]], "stale_in_cells": int(head[3]), "shared_free": bool(head[4]),
         "has_columns": [bool(head[5]), bool(head[6])], "n_ucol": [int(head[7]), int(head[8])]}
    off = 160
    for name, dt, cnt in [("code", np.uint16, head[9]), ("dead0", np.uint8, head[10]), ("dead1", np.uint8, head[11]), ("dead2", np.uint8, head[12]),
                          ("ucol0", np.uint16, head[13]), ("ucol1", np.uint16, head[14]), ("uflag0", np.uint32, head[15]),
                          ("uflag1", np.uint32, head[16]), ("bnd_idx", np.int32, head[17])]:
        t[name] = np.frombuffer(raw, dt, int(cnt), off)
        off += int(cnt) * np.dtype(dt).itemsize
    assert off == len(raw)
    return t


def shared_columns(code, dead, d, dimz):
    """ucol, uflag, n_ucol of direction d from the local codes [i][j][k] and dead[d] ([o][k])."""
    keep = (0xF << (4 * d)) | (3 << CODE_TYPE_SHIFT)
    cols = np.transpose(code & keep, (1, 2, 0) if d == 0 else (0, 2, 1))                 # [o][k][s]: the column of every line
    n_o, _, n = cols.shape
    ng = (dimz + 31) // 32
    pad = ng * 32 - dimz
    cols = np.pad(cols, ((0, 0), (0, pad), (0, 0))).reshape(n_o, ng, 32, n)
    live = np.pad(dead == 0, ((0, 0), (0, pad))).reshape(n_o, ng, 32)
    any_live = live.any(axis=2)
    first = live.argmax(axis=2)                                                           # first live line of the group
    col = np.take_along_axis(cols, first[:, :, None, None], axis=2)[:, :, 0, :] * any_live[..., None]
    uni = ((cols == col[:, :, None, :]).all(axis=3) | ~live).all(axis=2)                  # bit 0; an empty group is uniform
    # the partner (g + 1) of every even group; a last group without one pairs with nothing
    ge = np.arange(0, ng, 2)
    has_p = ge + 1 < ng
    gp = np.minimum(ge + 1, ng - 1)
    equal = (col[:, ge] == col[:, gp]).all(axis=2)
    pair = np.zeros((n_o, ng), bool)
    pair[:, ge] = uni[:, ge] & (~has_p | (uni[:, gp] & (~any_live[:, ge] | ~any_live[:, gp] | equal)))
    take = np.zeros((n_o, ng), bool)                                                      # all-dead even group, live partner, pair holds
    take[:, ge] = pair[:, ge] & has_p & ~any_live[:, ge] & any_live[:, gp]
    partner = np.roll(col, -1, axis=1)
    col = np.where(take[..., None], partner, col)
    # ids by first appearance over q = o * ng + g
    flat, u = col.reshape(n_o * ng, n), uni.reshape(-1)
    uflag = np.zeros(n_o * ng, np.uint32)
    ucol = np.zeros((1, UCOL_PITCH), np.uint16)
    n_ucol = 0
    if u.any():
        qs = np.flatnonzero(u)
        distinct, first_q, inv = np.unique(flat[qs], axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first_q)                      # distinct columns in the order of their first q
        rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
        ids = rank[inv.reshape(-1)]
        uflag[qs] = 1 | (pair.reshape(-1)[qs].astype(np.uint32) << 1) | (ids.astype(np.uint32) << 2)
        n_ucol = len(order)
        ucol = np.zeros((n_ucol, UCOL_PITCH), np.uint16)
        ucol[:, :n] = distinct[order]
    return ucol.reshape(-1), uflag, n_ucol


def restate(g, x0=0, nx=None):
    """Every table from the node arrays."""
    nx = g.dimx if nx is None else nx
    loc = slice(x0, x0 + nx)
    ty = g.type[loc]
    is_in = ty == grids.NODE_IN
    code = (ty.astype(np.uint16) & 3) << CODE_TYPE_SHIFT
    t = {"nseg": [], "stale_in_cells": 0, "shared_free": False}
    free = (g.bc_vel == grids.BC_FREE) | (g.bc_temp == grids.BC_FREE)
    for d in range(3):
        # X lines span all slabs: their kinds, their count and the refusal are those of the global line; Y and Z lines lie in a plane
        kind, shared = rule_kinds(g.type, d)
        own = slice(None) if d == 0 else loc
        nseg = int((kind[own] == ROW_START).sum())
        t["shared_free"] |= bool((shared & free)[own].any())
        kind = kind[loc]
        ends = (kind == ROW_START) | (kind == ROW_END)                                    # BC bits on START and END cells only
        rc = kind | (ends & (g.bc_vel[loc] == grids.BC_FREE)) * ROW_VELFREE | (ends & (g.bc_temp[loc] == grids.BC_FREE)) * ROW_TEMPFREE
        code |= (rc << (4 * d)).astype(np.uint16)
        t["nseg"].append(nseg)
        t["dead%d" % d] = (~is_in.any(axis=d)).astype(np.uint8).reshape(-1)               # the line has no NODE_IN cell
        t["stale_in_cells"] += int((is_in & (kind == ROW_SKIP)).sum())
    t["code"] = code.reshape(-1)
    t["bnd_idx"] = np.flatnonzero((ty == grids.NODE_BOUND) | (ty == grids.NODE_VALVE)).astype(np.int32)
    t["has_columns"] = [nx <= UCOL_PITCH, g.dimy <= UCOL_PITCH]
    t["n_ucol"] = [0, 0]
    for d in range(2):
        if t["has_columns"][d]:
            t["ucol%d" % d], t["uflag%d" % d], t["n_ucol"][d] = shared_columns(code, t["dead%d" % d].reshape(-1, g.dimz), d, g.dimz)
        else:
            t["ucol%d" % d], t["uflag%d" % d] = np.zeros(0, np.uint16), np.zeros(0, np.uint32)
    return t


ARRAYS = ("code", "dead0", "dead1", "dead2", "ucol0", "ucol1", "uflag0", "uflag1", "bnd_idx")
SCALARS = ("nseg", "stale_in_cells", "shared_free", "has_columns", "n_ucol")


def assert_tables(got, want):
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def oracle_nseg(g):
    from oracle import oracle as O
    o = O.Oracle(g, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)
    n = [o.num_segments(d) for d in range(3)]
    o.close()
    return n


def flag_bits(t, d, dimz):
    """uflag of direction d as [o][g] arrays: bit 0, bit 1, id."""
    f = t["uflag%d" % d].reshape(-1, (dimz + 31) // 32)
    return f & 1, (f >> 1) & 1, f >> 2


def check_single(program, tmp_path, g):
    got = run_builder(program, tmp_path, g)
    assert_tables(got, restate(g))
    assert got["nseg"] == oracle_nseg(g)
    return got


def test_box_with_a_partial_second_group(built, program, tmp_path):
    g = grids.box(12, 10, 40)                            # two groups, the second with 8 lines; face rows are all-dead groups
    t = check_single(program, tmp_path, g)
    b0, b1, ids = flag_bits(t, 0, 40)
    assert b0.all() and b1[:, 0].all() and not b1[:, 1].any()
    # two columns per direction: the one every live line carries, and the zeros of the all-dead groups of the face rows
    assert t["dead0"].reshape(10, 40)[0].all() and t["n_ucol"] == [2, 2] and t["stale_in_cells"] == 0


def test_obstacle_with_three_groups(built, program, tmp_path):
    g = grids.box_with_obstacle(20, 16, 70)              # the last even group has no partner; the obstacle breaks uniformity
    t = check_single(program, tmp_path, g)
    b0, b1, _ = flag_bits(t, 0, 70)
    assert not b0.all() and (b1[:, 2] == b0[:, 2]).all()


def test_pair_of_uniform_groups_with_different_columns(built, program, tmp_path):
    g = grids.box(10, 9, 64)
    sel = (slice(3, 6), slice(3, 6), slice(32, 63))
    g.type[sel] = grids.NODE_BOUND; g.bc_vel[sel] = grids.BC_NOSLIP; g.bc_temp[sel] = grids.BC_NOSLIP
    t = check_single(program, tmp_path, g)
    b0, b1, ids = flag_bits(t, 0, 64)
    assert b0[4].all() and b1[4, 0] == 0 and ids[4, 0] != ids[4, 1]          # row j = 4: both uniform, two ids, no pair


def test_runs_that_reach_the_end_of_the_x_line(built, program, tmp_path):
    g = grids.box(10, 9, 12)
    g.type[-1, 3:6, 3:6] = grids.NODE_IN
    t = check_single(program, tmp_path, g)
    assert t["stale_in_cells"] > 0
    assert t["nseg"][0] == 7 * 10 - 9                    # the nine X lines without a closing cell carry no segment


def test_y_lines_longer_than_a_column(built, program, tmp_path):
    g = grids.box(3, 513, 3)
    t = check_single(program, tmp_path, g)
    assert t["has_columns"] == [True, False] and len(t["ucol1"]) == 0 and len(t["uflag1"]) == 0 and len(t["ucol0"]) > 0


def test_shared_free_cell_is_reported(program, tmp_path):
    n = 8                                                # baffle_box(8) of tests/test_gpu_moving.py
    g = grids.box(n, n, n)
    g.type[n // 2, n // 3:2 * n // 3, n // 3:2 * n // 3] = grids.NODE_BOUND
    g.bc_temp[n // 2, n // 3:2 * n // 3, n // 3:2 * n // 3] = grids.BC_FREE
    t = run_builder(program, tmp_path, g)
    want = restate(g)
    assert t["shared_free"] is True and want["shared_free"] is True
    assert t["nseg"] == want["nseg"] and np.array_equal(t["code"], want["code"])      # what the builder had when it refused


def test_all_dead_even_group_takes_its_partners_column(built, program, tmp_path):
    g = grids.box(6, 6, 40)
    g.type[:, :, :32] = grids.NODE_OUT                   # group 0 of every row is dead, group 1 is live in the interior rows
    t = check_single(program, tmp_path, g)
    b0, b1, ids = flag_bits(t, 0, 40)
    assert t["dead0"].reshape(6, 40)[:, :32].all() and not t["dead0"].reshape(6, 40)[2, 32:39].any()
    assert b0[2].all() and b1[2, 0] == 1 and ids[2, 0] == ids[2, 1]
    assert t["ucol0"].reshape(-1, UCOL_PITCH)[ids[2, 0]].any()


def test_slabs_cut_the_single_context_tables(built, program, tmp_path):
    g = grids.box_with_obstacle(20, 16, 40)
    whole = run_builder(program, tmp_path, g)
    assert_tables(whole, restate(g))
    plane = 16 * 40
    nseg_yz = [0, 0]
    for x0, nx in ((0, 7), (7, 6), (13, 7)):
        t = run_builder(program, tmp_path, g, x0, nx)
        assert_tables(t, restate(g, x0, nx))             # dead[0] and the X columns: the definitions on the local planes
        assert np.array_equal(t["code"], whole["code"][x0 * plane:(x0 + nx) * plane])
        assert np.array_equal(t["dead1"], whole["dead1"][x0 * 40:(x0 + nx) * 40])
        assert np.array_equal(t["dead2"], whole["dead2"][x0 * 16:(x0 + nx) * 16])
        assert t["nseg"][0] == whole["nseg"][0]
        nseg_yz[0] += t["nseg"][1]; nseg_yz[1] += t["nseg"][2]
    assert nseg_yz == whole["nseg"][1:]
