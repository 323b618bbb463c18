"""The extrusion of a Shape2D grid on the device, the parts that need no GPU: the C-ABI entries exist, the per-cell priority rule
(shape2d.extrude_shape2d -- what the kernel k_geom_extrude implements) gives the nodes of the loop it restates on every case of
tests/extrude_cases.py, the C++ host function ExtrudeShape2D agrees on the degenerate ones, and the library's per-column `bottom`
table equals the twin's.  Everything is array_equal: the extrusion moves bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_decls
import extrude_cases as EC
from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids, shape2d

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("fs3d_extrude_shape2d_dev", "fs3d_update_nodes_shape2d", "fs3d_shape2d_bottom")


@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


def test_header_declares_and_library_exports_the_extrusion_entries(built):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert hasattr(capi.Solver, "extrude_shape2d_dev") and hasattr(capi.Solver, "update_nodes_shape2d")


@pytest.mark.parametrize("case", EC.CASE_IDS)
def test_priority_rule_equals_the_loop(case):
    nodes, g2, p = EC.load_case(case)
    EC.assert_nodes_equal(EC.twin(g2, p), nodes)


def test_the_cases_reach_every_rule():
    """The case list is worth its name: over it the middle holds all three column types (a valve at rest and a moving one), the
    floor reaches the bound and the lid, k = 0 carries the bound's values (active_dimz 2), and a ragged dimz occurs."""
    seen = set()
    for case in EC.CASE_IDS:
        nodes, g2, p = EC.load_case(case)
        A = shape2d.active_dimz_of(p["dz"], p["depth"])
        bottom = shape2d.bottom_table(g2.dimx, g2.dimy, A, p["depth_var"])
        live = g2.cell != grids.NODE_OUT
        if nodes.dimz % 4:
            seen.add("ragged")
        if A == 2 and (nodes.bc_temp[:, :, 0][live] == grids.BC_FREE).all() and (nodes.type[:, :, 0] == grids.NODE_OUT).all():
            seen.add("k0-keeps-the-bound")
        if (bottom[live] == A - 2).any():
            seen.add("floor-reaches-bound")
        if (bottom[live] >= A - 1).any() and (nodes.type[:, :, A - 1][live & (bottom >= A - 1)] == grids.NODE_BOUND).all():
            seen.add("floor-enters-lid")
        if (bottom[live] + 1 < A - 2).any():
            mid = nodes.type[:, :, A - 3][live & (bottom + 1 < A - 2)]
            seen |= {"middle-%d" % t for t in np.unique(mid)}
            if (nodes.bc_vel[:, :, A - 3][g2.cell == grids.NODE_VALVE] == grids.BC_FREE).any():
                seen.add("valve-at-rest")
            if (nodes.bc_vel[:, :, A - 3][g2.cell == grids.NODE_VALVE] == grids.BC_NOSLIP).any():
                seen.add("valve-moving")
    assert seen >= {"ragged", "k0-keeps-the-bound", "floor-reaches-bound", "floor-enters-lid", "middle-0", "middle-2", "middle-3",
                    "valve-at-rest", "valve-moving"}, seen


def _grid_dump(path):
    raw = open(path, "rb").read()
    nx, ny, nz, esz = (int(v) for v in np.frombuffer(raw[:16], np.int32))
    n, off, out = nx * ny * nz, 16, {}
    for name in ("type", "bc_vel", "bc_temp"):
        out[name] = np.frombuffer(raw[off:off + n], np.uint8).reshape(nx, ny, nz); off += n
    dt = np.float32 if esz == 4 else np.float64
    for name in ("vx", "vy", "vz", "T"):
        out[name] = np.frombuffer(raw[off:off + n * esz], dt).reshape(nx, ny, nz); off += n * esz
    assert off == len(raw)
    return out


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("case", [c[0] for c in EC.DEGENERATE])
def test_cpp_host_function_accepts_the_degenerate_cases_and_equals_the_rule(driver, case, prec, tmp_path):
    """fs3d_run --grid-only: ExtrudeShape2D itself on the authored outline (no GPU), against the priority rule."""
    nodes, g2, p = EC.load_case(case)
    data, cfgf, dump = str(tmp_path / "outline_2D_data.txt"), str(tmp_path / "outline_2D_config.txt"), str(tmp_path / "grid.bin")
    open(data, "w").write(EC.OUTLINE)
    open(cfgf, "w").write(EC.config_text(p))
    args = [driver, data, str(tmp_path / "o"), cfgf] + (["align"] if p["align"] else []) + ["--grid-only", dump] + (["double"] if prec == "double" else [])
    subprocess.run(args, check=True, capture_output=True, text=True)
    g, want = _grid_dump(dump), EC.twin(g2, p)
    assert g["type"].shape == tuple(want.shape)
    dt = np.float32 if prec == "float" else np.float64
    for name in EC.NODE_ARRAYS:
        a, b = g[name], np.asarray(getattr(want, name), g[name].dtype)
        assert name in ("type", "bc_vel", "bc_temp") or a.dtype == dt
        assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), name


@pytest.mark.parametrize("case", ["heart_us-t0", "non_uniform_pipe", "u_bend", "adz5-var3-align", "adz5-var1-ragged", "adz2-var3-ragged"])
def test_library_bottom_table_equals_the_twin(built, case):
    nodes, g2, p = EC.load_case(case)
    A = shape2d.active_dimz_of(p["dz"], p["depth"])
    got = capi.shape2d_bottom(g2.dimx, g2.dimy, p["dz"], p["depth"], p["depth_var"])
    want = shape2d.bottom_table(g2.dimx, g2.dimy, A, p["depth_var"])
    assert got.dtype == np.int32 and np.array_equal(got, want)
    # ... and the loop's own (python floats, cell by cell), which the twin vectorises
    h = max(A - 4, 0)
    loop = [[1 + int(p["depth_var"] * (1.0 - ((-1 + 2 * float(i) / g2.dimx) ** 2 + (-1 + 2 * float(j) / g2.dimy) ** 2) * 0.5) * h)
             for j in range(g2.dimy)] for i in range(0, g2.dimx, 7)]
    assert np.array_equal(want[::7], np.array(loop))
    if p["depth_var"] and h:
        assert len(np.unique(want)) > 1


@pytest.mark.parametrize("word", ["--host-extrusion", "--time-geometry"])
def test_driver_refuses_the_moving_words_without_moving(driver, word, tmp_path):
    data, cfgf = (os.path.join(HERE, "golden", "inputs", f) for f in ("heart_us_2D_data.txt", "heart_us_2D_config.txt"))
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "GPU", word], capture_output=True, text=True)
    assert r.returncode != 0 and "Caught exception" in r.stderr and word + ": only with moving" in r.stderr


def test_bottom_table_refuses_what_gives_no_active_dimz(built):
    lib = capi.load()
    out = (C.c_int * 4)()
    for dz, depth in ((0.0, 1.0), (-1.0, 1.0), (1.0, -1.0), (1e-9, 1.0), (float("nan"), 1.0)):
        assert lib.fs3d_shape2d_bottom(2, 2, dz, depth, 0.0, out) == capi.ERR_INVALID
    assert lib.fs3d_shape2d_bottom(2, 2, 1.0, 1.0, 0.0, None) == capi.ERR_INVALID
    assert lib.fs3d_shape2d_bottom(0, 2, 1.0, 1.0, 0.0, out) == capi.ERR_INVALID


def test_rule_refuses_what_the_loop_cannot_hold():
    nodes, g2, p = EC.load_case("adz5-var3-ragged")
    with pytest.raises(ValueError):
        shape2d.extrude_grid2d(g2, p["dz"], p["depth"], 30.0, p["baseT"], False)       # bottom far above dimz
    with pytest.raises(ValueError):
        shape2d.extrude_grid2d(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"], False, dimz=4)   # active_dimz 5 > dimz
