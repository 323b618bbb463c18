"""Moving Shape3D meshes on x-slabs, the parts that need no GPU: include/fs3d.h declares the entries, capi.SYMBOLS binds them
with their twins' arguments and the library exports them, the driver refuses --slab-voxels where it means nothing, and the cases
of tests/mesh_slab_cases.py can show what the GPU tests use them for."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import abi_decls  # noqa: E402
import mesh_slab_cases as MS  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids  # noqa: E402

INPUTS = os.path.join(HERE, "golden", "inputs")
SPHERE = ("sphere_3D_data.txt", "sphere_3D_config.txt")
ENTRIES = {"fs3d_update_nodes_shape3d_slab", "fs3d_update_nodes_shape3d_vel_slab", "fs3d_flood_fill_global_dev"}


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------

def test_the_header_declares_and_the_binding_binds_the_entries():
    for name in sorted(ENTRIES):
        assert abi_decls.declares_status(name), name
        assert name in capi.SYMBOLS, name


def test_the_library_exports_the_entries_with_their_twins_arguments(built):
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in sorted(ENTRIES):
        assert hasattr(lib, name), "libfs3d_hip.so does not export %s" % name
        assert getattr(capi.load(), name).argtypes == capi.SYMBOLS[name][1]
    declared = abi_decls.functions()
    for entry, twin in (("fs3d_update_nodes_shape3d_slab", "fs3d_update_nodes_shape3d"),
                        ("fs3d_update_nodes_shape3d_vel_slab", "fs3d_update_nodes_shape3d_vel"),
                        ("fs3d_flood_fill_global_dev", "fs3d_flood_fill_dev")):
        assert capi.SYMBOLS[entry] == capi.SYMBOLS[twin] and declared[entry] == declared[twin], entry


def test_the_solver_class_has_the_methods():
    for name in ("update_nodes_shape3d_slab", "update_nodes_shape3d_vel_slab", "flood_fill_global_dev"):
        assert callable(getattr(capi.Solver, name))


# ---- the driver's argument errors -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


def refused(driver, tmp_path, words):
    data, cfgf = (os.path.join(INPUTS, f) for f in SPHERE)
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align"] + words, capture_output=True, text=True)
    assert r.returncode != 0 and "Caught exception" in r.stderr, r.stderr
    return r.stderr


def test_driver_refuses_slab_voxels_without_moving_mesh(driver, tmp_path):
    err = refused(driver, tmp_path, ["GPU", "2", "--same-device", "--slab-voxels"])
    assert "--slab-voxels: only with moving-mesh" in err


@pytest.mark.parametrize("gpu", [["GPU"], ["GPU", "1"]], ids=["GPU", "GPU-1"])
def test_driver_refuses_slab_voxels_on_one_gpu(driver, tmp_path, gpu):
    err = refused(driver, tmp_path, gpu + ["moving-mesh", "--slab-voxels"])
    assert "--slab-voxels: only with GPU n for n > 1" in err


def test_driver_refuses_both_voxel_words(driver, tmp_path):
    err = refused(driver, tmp_path, ["GPU", "2", "moving-mesh", "--slab-voxels", "--host-voxels"])
    assert "--slab-voxels: not together with --host-voxels" in err


def test_the_refusal_of_plain_moving_mesh_on_slabs_names_both_words(driver, tmp_path):
    err = refused(driver, tmp_path, ["GPU", "2", "--same-device", "moving-mesh"])
    assert "the host voxelisation works on x-slabs" in err and "--host-voxels" in err and "--slab-voxels" in err


def test_the_usage_line_names_the_word(driver):
    r = subprocess.run([driver], capture_output=True, text=True)
    assert "--slab-voxels" in r.stdout


# ---- the conditions of the cases ------------------------------------------------------------------------------------------------------------

def test_reference_cases_have_the_dims_they_are_there_for():
    a, b = MS.case("sphere-t2").want, MS.case("sphere-ragged").want
    assert a.shape == (32, 32, 32) and b.shape == (25, 24, 25) and b.dimz % 4 != 0
    x0, x1 = MS.ranges(a.dimx, 4)[3]                       # the last of four slabs: no wall and no fluid cell, and it has to work too
    assert not np.isin(a.type[x0:x1], (grids.NODE_IN, grids.NODE_BOUND)).any()
    for c in (a, b):
        assert c.count(grids.NODE_IN) > 0 and c.count(grids.NODE_BOUND) > 0


def test_every_slab_of_the_velocity_case_holds_fluid_and_moving_walls():
    want = MS.case("sphere-80-vel").want
    assert want.shape == (64, 81, 64)
    fewest_in, fewest_moving = None, None
    for nranks in (2, 3, 4):
        for x0, x1 in MS.ranges(want.dimx, nranks):
            n_in = int((want.type[x0:x1] == grids.NODE_IN).sum())
            wall = want.type[x0:x1] == grids.NODE_BOUND
            speed2 = np.asarray(want.vx[x0:x1]) ** 2 + np.asarray(want.vy[x0:x1]) ** 2 + np.asarray(want.vz[x0:x1]) ** 2
            moving = int((wall & (speed2 > 0)).sum())
            print(nranks, (x0, x1), n_in, moving)
            assert n_in > 0 and moving > 0, (nranks, x0, x1)
            fewest_in = n_in if fewest_in is None else min(fewest_in, n_in)
            if x0 > 0:
                fewest_moving = moving if fewest_moving is None else min(fewest_moving, moving)
    assert (fewest_in, fewest_moving) == (5986, 2607)
    assert (want.T[want.type == grids.NODE_BOUND] == np.float32(WV.WALL_T)).all()


def test_the_zero_case_is_the_plain_entrys_grid():
    z, v = MS.case("sphere-80-zero"), MS.case("sphere-80-vel")
    assert np.array_equal(z.want.type, v.want.type) and not np.asarray(z.want.vx).any() and not z.vel.any() and z.wallT == 0.0
    assert (z.want.T[z.want.type == grids.NODE_BOUND] == 0).all()


def test_a_slab_local_fill_would_show_in_the_tube_case():
    c = MS.case("tube-cube")
    ty = c.want.type
    assert ty.shape == MS.TUBE_DIMS and len(c.idx) == 8 + 12
    assert MS.ranges(ty.shape[0], 3)[1] == MS.TUBE_SLAB
    assert int((ty == grids.NODE_IN).sum()) == 8 and int((ty == grids.NODE_BOUND).sum()) == 632
    x0, x1 = MS.TUBE_SLAB
    n_global = int((ty[x0:x1] == grids.NODE_IN).sum())
    n_local = int((MS.slab_local_fill(ty, MS.TUBE_SLAB) == grids.NODE_IN).sum())
    assert (n_global, n_local) == (8, 456) and n_global < n_local
    assert (ty[11:13, 7:9, 7:9] == grids.NODE_IN).all()        # the cube's inside


def test_the_translating_sphere_crosses_the_slab_cuts():
    steps = WV.translating_grids()
    assert steps[0][0].shape == (28, 35, 28) and len(steps) == 8
    for nranks, first, last in ((2, 506, 1371), (3, 0, 252)):
        x0, x1 = MS.ranges(28, nranks)[-1]
        got = [int((steps[k][0].type[x0:x1] == grids.NODE_IN).sum()) for k in (0, -1)]
        assert got == [first, last], (nranks, got)
