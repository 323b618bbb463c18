"""Moving Shape3D meshes, the parts that need no GPU: the sub-frame of a mesh at a time t is what build() makes the grid of time t
from (Python twin and C++ host, the latter held to the reference's own grids), the driver's --grid-only --grid-time works for a
Shape3D input, and the flood fill as directional passes repeated to a fixed point -- the algorithm of the device kernels -- gives
the connected component scipy labels."""
import os
import subprocess

import numpy as np
import pytest

import mesh_cases as MC
import refgolden as RG
from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import grids, shape3d
from test_moving_api import _grid_dump

INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")


@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


@pytest.mark.parametrize("ti", range(5))
def test_subframe_then_build_is_the_grid_of_that_time(ti):
    t = MC.fx_times()[ti]
    want, fx = MC.twin("sphere_3D", time=t)
    sh, _ = MC.twin("sphere_3D")
    g, idx = sh.subframe(t)
    assert g.dtype == np.float32 and g.shape == (len(sh.frames[0]["v"]), 3) and idx.shape[1] == 3
    sh.build(g, idx)
    assert np.array_equal(sh.type, want.type)
    assert np.array_equal(sh.type, fx.z["grid%d_type" % ti])
    if ti in (1, 2, 3):      # 0.1, 0.2, 0.3 s fall inside a frame (0.0 and 0.5 s on multiples of the 1/75 s frame length): the walls have moved
        assert not np.array_equal(sh.type, MC.twin("sphere_3D")[0].type)


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("ti", range(5))
def test_cpp_grid_at_time_t_equals_the_twin_and_the_reference(driver, ti, prec, tmp_path):
    """--grid-only F --grid-time t for a Shape3D input: SubFrame(t) + Build in host/Shape3D.h -- the grid `moving-mesh --host-voxels`
    uploads at time t, and the one the device voxeliser must give."""
    t = MC.fx_times()[ti]
    want, fx = MC.twin("sphere_3D", time=t)
    dump = str(tmp_path / "grid.bin")
    args = [driver, fx.data_path, str(tmp_path / "out"), os.path.join(INPUTS, "sphere_3D_config.txt"), "align", "--grid-only", dump, "--grid-time", repr(float(t))]
    subprocess.run(args + (["double"] if prec == "double" else []), check=True, capture_output=True, text=True)
    g = _grid_dump(dump)
    nodes = MC.nodes_of(want)
    for name in ("type", "bc_vel", "bc_temp"):
        assert np.array_equal(g[name], getattr(nodes, name)), name
    dt = np.float32 if prec == "float" else np.float64
    for name in ("vx", "vy", "vz", "T"):
        assert g[name].dtype == dt and np.array_equal(g[name], np.asarray(getattr(nodes, name), dt)), name
    assert np.array_equal(g["type"], fx.z["grid%d_type" % ti])


def test_directional_passes_to_a_fixed_point_give_the_labelled_component():
    for name, ty in MC.fill_grids().items():
        got, rounds = MC.pass_fill(ty)
        want = MC.label_fill(ty)
        print(name, ty.shape, "rounds", rounds, "NODE_OUT", int((want == grids.NODE_OUT).sum()))
        assert np.array_equal(got, want), name
        if name == "all-in":
            assert (want == grids.NODE_OUT).all()
        if name == "serpentine":      # the maze is what makes the fill iterate, and it keeps fluid the fill must not reach
            assert rounds > 8 and (want == grids.NODE_IN).any() and (want[:-4] == grids.NODE_OUT).sum() > want[:-4].size // 3
        if name == "bound-at-origin":
            assert want[0, 0, 0] == grids.NODE_OUT and (want[5:] == grids.NODE_IN).all()
        if name == "two-shells":
            assert want[3, 3, 3] == grids.NODE_IN and want[8, 8, 8] == grids.NODE_IN and want[0, 5, 5] == grids.NODE_OUT


def test_twin_raises_on_the_scan_line_the_device_refuses():
    sh2, _ = MC.twin("sphere_3D")
    with pytest.raises(ValueError, match="never reaches its end cell"):
        sh2.build(*MC.long_scan_line_mesh())
