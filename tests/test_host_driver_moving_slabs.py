"""fs3d_run with a moving geometry on x-slabs (`moving` / `moving-mesh --host-voxels` together with `GPU n`): rank 0 prepares the
geometry of each step on the host, every slab rebuilds the tables of its own planes from it (fs3d_update_nodes_slab,
fs3d_update_nodes_shape2d_slab).  The err prints and the records of `_res.nc` equal the single-GPU run's value for value; all
slabs sit on device 0 (--same-device)."""
import os
import re
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
HEART = ("heart_us_2D_data.txt", "heart_us_2D_config.txt")
SPHERE = ("sphere_3D_data.txt", "sphere_3D_config.txt")
VARS = ("u", "v", "w", "T", "time")


@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


def run(driver, tmp_path, tag, case, words):
    """(err prints, {variable: records}) of one run on the bit-exact kernels."""
    from scipy.io import netcdf_file
    data, cfgf = (os.path.join(INPUTS, f) for f in case)
    prefix = str(tmp_path / tag)
    r = subprocess.run([driver, data, prefix, cfgf, "align"] + words, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    f = netcdf_file(prefix + "_res.nc", "r", mmap=False)
    rec = {v: np.array(f.variables[v][:]) for v in VARS}
    f.close()
    return re.findall(r"err = ([0-9.]+),", r.stdout), rec


def assert_same_run(one, other, steps):
    assert len(one[0]) == steps and one[0] == other[0]
    assert one[1]["u"].shape[0] >= 1
    for v in VARS:
        np.testing.assert_array_equal(one[1][v], other[1][v])


@pytest.fixture(scope="module")
def heart_single(driver, tmp_path_factory):
    return run(driver, tmp_path_factory.mktemp("heart"), "one", HEART, ["GPU", "moving", "--steps", "12"])


@pytest.mark.parametrize("words", [["GPU", "2", "--same-device", "moving"], ["GPU", "3", "--same-device", "moving"],
                                   ["GPU", "2", "--same-device", "moving", "--host-extrusion"]], ids=lambda w: "-".join(w[1:]))
def test_moving_on_slabs_equals_the_single_gpu_run(driver, heart_single, words, tmp_path):
    assert_same_run(heart_single, run(driver, tmp_path, "slabs", HEART, words + ["--steps", "12"]), 12)


def test_moving_mesh_with_host_voxels_on_slabs_equals_the_single_gpu_run(driver, tmp_path):
    words = ["moving-mesh", "--host-voxels", "--watertight", "--wall-velocity", "motion", "--steps", "6"]
    one = run(driver, tmp_path, "one", SPHERE, ["GPU"] + words)
    assert_same_run(one, run(driver, tmp_path, "slabs", SPHERE, ["GPU", "2", "--same-device"] + words), 6)


def test_moving_mesh_on_slabs_needs_the_host_voxelisation(driver, tmp_path):
    data, cfgf = (os.path.join(INPUTS, f) for f in SPHERE)
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfgf, "align", "GPU", "2", "--same-device", "moving-mesh"], capture_output=True, text=True)
    assert r.returncode != 0 and "Caught exception" in r.stderr
    assert "moving-mesh" in r.stderr and "the host voxelisation works on x-slabs" in r.stderr and "--host-voxels" in r.stderr
