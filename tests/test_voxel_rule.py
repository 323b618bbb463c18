"""CPU: the shared voxel rule (cmc_fluid_solver_amd/csrc/fs3d_voxel.h: set-up, column, cell test, wall velocity -- what the kernels and
the host loader both run) in a stand-alone program built with the address and undefined-behaviour sanitizers, without the loader:
the wall bytes before any fill, the owners and the float64 wall velocities equal the twin's (shape3d.Shape3D.build with
velocities) exactly, with the conservative and with the thin shell."""
import os
import subprocess

import numpy as np
import pytest

import thin_shell_cases as TS
import wall_velocity_cases as WV
import watertight_cases as W
from cmc_fluid_solver_amd import capi, grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sphere-20", "tetra", "box_pipe_3D", "outside", "degenerate"] + list(W.DEGENERATE_ROTATED)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("voxel_rule") / "voxel_rule_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", os.path.join(ROOT, "tests", "voxel_rule_test.cpp"), "-o", exe])
    return exe


def test_rotated_degenerate_meshes_have_their_depth_along_every_axis():
    """what the rotated cases are for: over the three meshes a degenerate triangle takes each of x, y, z as its depth axis"""
    depth = {}
    for case in ["degenerate"] + list(W.DEGENERATE_ROTATED):
        sh, g, idx, _ = W.gpu_case(case)
        setups = [sh._voxel_setup(tuple(tuple(np.float32(c) for c in g[v]) for v in t)) for t in idx]
        assert all(st[4] is None for st in setups)            # (no plane: every triangle is degenerate)
        depth[case] = {st[2][2] for st in setups}
    # smallest extent along old z -> new y, new x; a tie (the point, the segment on cell planes) takes x under every rotation
    assert depth == {"degenerate": {0, 2}, "degenerate-yzx": {0, 1}, "degenerate-zxy": {0}}


@pytest.mark.parametrize("case", CASES)
def test_sanitized_rule_equals_the_twin(program, tmp_path, case):
    sh, g, idx = WV.mesh(case)
    vel = WV.velocities(g)
    src, dst = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    xyz, tri = capi.Solver._mesh_arrays(g, idx)
    with open(src, "wb") as f:
        np.array(list(sh.type.shape) + [len(g), len(idx)], np.int32).tofile(f)
        for a in xyz + [np.ascontiguousarray(vel[:, c]) for c in range(3)] + [tri]:
            a.tofile(f)
    for shell, twin in ((0, WV.built(sh, g, idx, vel)), (1, TS.thin(sh, g, idx, vel))):
        r = subprocess.run([program, src, dst, str(shell)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        n = sh.type.size
        wall = np.fromfile(dst, np.uint8, n).reshape(sh.type.shape)
        own = np.fromfile(dst, np.int32, n, offset=n).reshape(sh.type.shape)
        u = np.fromfile(dst, np.float64, 3 * n, offset=5 * n).reshape((3,) + sh.type.shape)
        assert wall.any() and np.array_equal(wall == 1, twin.type == grids.NODE_BOUND), "shell %d: %d cells differ" % (shell, int(((wall == 1) != (twin.type == grids.NODE_BOUND)).sum()))
        assert np.array_equal(own, twin.owner), "shell %d: %d owners differ" % (shell, int((own != twin.owner).sum()))
        for c in range(3):
            assert np.array_equal(u[c].view(np.uint64), twin.wall_v[c].view(np.uint64)), "shell %d, component %d: %d velocities differ" % (shell, c, int((u[c] != twin.wall_v[c]).sum()))
        assert any(twin.wall_v[c].any() for c in range(3))
