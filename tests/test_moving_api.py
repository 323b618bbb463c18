"""Moving geometry, the parts that need no GPU: the four C-ABI entries exist, the local row-kind rule the device kernels use
(kernels_geom.hip) gives the CPU oracle's segment lists, the C++ re-extrusion at a time t equals its Python twin (which
tests/test_ref_golden.py pins to the reference's grids at the same times), and the driver refuses `moving` where it cannot move."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_decls
import refgolden as RG
from geom_rules import rule_segments
from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids, shape2d

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
NEW = ("fs3d_update_nodes", "fs3d_update_nodes_dev", "fs3d_clear_outer_cells", "fs3d_geometry_info")


@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


def heart_nodes(t, fx=None):
    fx = fx or RG.Fixture("heart_us", "f32")
    cfg = fx.cfg()
    return shape2d.load_shape2d(fx.data_path, cfg.dx, cfg.dy, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT, fx.meta["align"], time=t)[0]


def test_header_declares_and_library_exports_the_moving_entries(built):
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert abi_decls.defines()["FS3D_N_GEOM_INFO"] == 14
    assert len(capi.Solver.GEOMETRY_INFO) == 14


def check_rule_against_oracle(nodes):
    from oracle import oracle as O
    o = O.Oracle(nodes, capi.fluid_params(np.float32, 200.0, 0.72, 1.4), np.float32)
    for d in range(3):
        want = o.segments(d)
        got = rule_segments(nodes.type, d)
        assert len(got) == len(want) == o.num_segments(d), (d, len(got), len(want))
        assert got == {((s[0], s[1], s[2]), (s[3], s[4], s[5])) for s in want}, d
        assert all(s[6] == (s[3] - s[0]) + (s[4] - s[1]) + (s[5] - s[2]) + 1 for s in want)
    o.close()


def test_row_kind_rule_gives_the_oracle_segments_on_the_box_with_obstacle(built):
    check_rule_against_oracle(grids.box_with_obstacle(20, 16, 18))


@pytest.mark.parametrize("ti", range(6))
def test_row_kind_rule_gives_the_oracle_segments_on_heart_us(built, ti):
    fx = RG.Fixture("heart_us", "f32")
    check_rule_against_oracle(heart_nodes(fx.meta["grid_times"][ti], fx))


def _grid_dump(path):
    raw = open(path, "rb").read()
    nx, ny, nz, esz = np.frombuffer(raw[:16], np.int32)
    n = nx * ny * nz
    off = 16
    out = {}
    for name in ("type", "bc_vel", "bc_temp"):
        out[name] = np.frombuffer(raw[off:off + n], np.uint8).reshape(nx, ny, nz); off += n
    dt = np.float32 if esz == 4 else np.float64
    for name in ("vx", "vy", "vz", "T"):
        out[name] = np.frombuffer(raw[off:off + n * esz], dt).reshape(nx, ny, nz); off += n * esz
    assert off == len(raw)
    return out


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("ti", range(6))
def test_cpp_re_extrusion_at_time_t_equals_the_python_loader(driver, ti, prec, tmp_path):
    """--grid-only F --grid-time t: load, Grid2D::Prepare(t), ExtrudeShape2D again -- the grid the moving loop uploads at time t."""
    fx = RG.Fixture("heart_us", "f32")
    t = fx.meta["grid_times"][ti]
    data, cfgf = fx.data_path, os.path.join(INPUTS, "heart_us_2D_config.txt")
    dump = str(tmp_path / "grid.bin")
    args = [driver, data, str(tmp_path / "out"), cfgf, "align", "--grid-only", dump, "--grid-time", repr(float(t))]
    subprocess.run(args + (["double"] if prec == "double" else []), check=True, capture_output=True, text=True)
    nodes = heart_nodes(t, fx)
    g = _grid_dump(dump)
    assert g["type"].shape == tuple(nodes.shape)
    for name in ("type", "bc_vel", "bc_temp"):
        assert np.array_equal(g[name], getattr(nodes, name)), name
    dt = np.float32 if prec == "float" else np.float64
    for name in ("vx", "vy", "vz", "T"):
        assert g[name].dtype == dt and np.array_equal(g[name], np.asarray(getattr(nodes, name), dt)), name
    if ti > 0:      # the walls do move: the dump is not the grid of time 0
        assert not np.array_equal(g["type"], heart_nodes(0.0, fx).type)


def test_driver_refuses_moving_for_a_shape3d_input(driver, tmp_path):
    data, cfgf = (os.path.join(INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "GPU", "moving"], capture_output=True, text=True)
    assert r.returncode != 0
    assert "Caught exception" in r.stderr and "moving: only in_fmt Shape2D inputs move" in r.stderr and "Shape3D" in r.stderr


def test_driver_refuses_moving_on_several_gpus(driver, tmp_path):
    data, cfgf = (os.path.join(INPUTS, f) for f in ("heart_us_2D_data.txt", "heart_us_2D_config.txt"))
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "GPU", "2", "moving"], capture_output=True, text=True)
    assert r.returncode != 0 and "moving: single GPU only" in r.stderr
