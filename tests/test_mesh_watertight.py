"""CPU: the conservative Shape3D voxeliser (voxels="conservative", fs3d_run --watertight, FS3D_OPT_MESH_VOXELS).
The twin (cmc_fluid_solver_amd/shape3d.py) is held to closedness on the meshes the default rasteriser leaks on and to a float64
separating-axis test that shares nothing with its loops (tests/watertight_cases.py); the C++ loader (host/Shape3D.h) is held to the
twin cell for cell through the driver and through a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_decls
import mesh_cases as MC
import watertight_cases as W
from test_shape3d import CONFIG, _grid_dump, icosphere
from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids, shape3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")


# ---- closedness -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("faces", [20, 80, 320])
def test_conservative_grid_is_closed_where_the_default_leaks(faces):
    """r = s (30, 38, 30), s = 0.5 .. 1.0 in 21 steps: closed at every scale; the default rasteriser has no NODE_IN cell at 8, 8
    and 2 of them (for 320 faces: s = 0.7 and 0.9)."""
    leaks = []
    for s in W.SCALES:
        r = tuple(s * x for x in (30, 38, 30))
        sh, cell = W.sphere(faces, r)
        W.assert_closed(W.closed_report(sh.type, cell))
        if not (W.sphere(faces, r, "reference")[0].type == grids.NODE_IN).any():
            leaks.append(round(s, 3))
    print(faces, "faces: the default leaks at", leaks)
    assert len(leaks) == W.LEAK_COUNT[faces]
    if faces == 320:
        assert leaks == W.LEAKS_320
    if faces == 80:
        assert 1.0 in leaks and 0.925 in leaks          # the two ends of the breathing run of tests/test_gpu_mesh_watertight.py


@pytest.mark.parametrize("faces,r,dims", W.SINGLE)
def test_single_leaking_spheres_are_closed(faces, r, dims):
    sh, cell = W.sphere(faces, r)
    assert sh.type.shape == dims
    W.assert_closed(W.closed_report(sh.type, cell))
    assert not (W.sphere(faces, r, "reference")[0].type == grids.NODE_IN).any()
    nodes = shape3d.nodes_of(sh, W.H, W.H, W.H, 1.0)       # the node arrays as with the default: NOSLIP, v = 0, T = 0 on the shell
    assert (nodes.T[sh.type == grids.NODE_BOUND] == 0).all() and (nodes.T[sh.type != grids.NODE_BOUND] == 1).all()
    assert (nodes.bc_vel == grids.BC_NOSLIP).all() and not nodes.vx.any()


def test_defaults_and_keyword():
    txt, _ = W.sphere_text(20, (15, 19, 15))
    a, _ = shape3d.load_shape3d(txt, W.H, W.H, W.H, align=False, is_text=True)
    b, _ = shape3d.load_shape3d(txt, W.H, W.H, W.H, align=False, is_text=True, voxels="reference")
    c, sh = shape3d.load_shape3d(txt, W.H, W.H, W.H, align=False, is_text=True, voxels="conservative")
    assert np.array_equal(a.type, b.type) and not np.array_equal(a.type, c.type) and sh.voxels == "conservative"
    assert ((a.type == grids.NODE_BOUND) <= (c.type == grids.NODE_BOUND)).mean() > 0.95      # (the default's shell is not a subset: it truncates)
    with pytest.raises(ValueError):
        shape3d.Shape3D(shape3d.parse_shape3d(txt), W.H, W.H, W.H, False, voxels="thin")
    big = W.blank((8, 8, 8))
    with pytest.raises(ValueError, match="4096"):
        big.build(np.array([[1, 1, 1], [2, 5000, 1], [3, 1, 2]], np.float32), np.array([[0, 1, 2]]))


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------

RESTATED = ["sphere-20", "box_pipe_3D", "tetra", "outside"]


@pytest.fixture(scope="module")
def restated():
    return {c: W.restatement(*W.gpu_case(c)[:3]) for c in RESTATED + ["degenerate"]}


@pytest.mark.parametrize("case", RESTATED + ["degenerate"])
def test_twin_equals_the_float64_overlap_test(restated, case):
    shell, missing, extra, free = restated[case]
    print(case, "shell %d cells, %d missing, %d extra, %d free (tolerance %.3g)" % (shell, missing, extra, free, W.tolerance(*W.gpu_case(case)[1:3])))
    assert shell > 0 and missing == 0 and extra == 0


@pytest.mark.parametrize("case", RESTATED)
def test_free_cells_are_below_one_percent_of_the_shell(restated, case):
    """Free: neither touching (float64, margin >= 0) nor separated by more than the tolerance (slack + rounding bound,
    shape3d.VOXEL_TOL * L: about 6e-9 of a cell on these meshes).  tetra is the case that needs it this small: its fourth vertex has
    the grid coordinate 21.000002 (fp32 of the file's value through the bounding box), so the face 5x + 6y + 10z = 526 passes
    within 1e-6 of 172 cell corners it would touch exactly -- 1.12 % of the shell, which no fp32 evaluation can tell from touching."""
    shell, missing, extra, free = restated[case]
    print(case, "free %d of %d = %.3f %%" % (free, shell, 100.0 * free / shell))
    assert free < 0.01 * shell


# ---- degenerate triangles ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(W.DEGENERATE))
def test_degenerate_triangle_sets_the_cells_of_its_longest_edge(name):
    tri, seg = W.DEGENERATE[name]
    sh = W.blank(W.DEGENERATE_DIMS)
    g = np.array(tri, np.float32)
    sh.build(g, np.array([[0, 1, 2]]))                       # nothing raises
    got = sh.type == grids.NODE_BOUND
    edge = np.array([seg[0], seg[1], seg[1]], np.float64)
    must = W.sat_overlap(W.DEGENERATE_DIMS, edge, [[0, 1, 2]], 0.0)
    may = W.sat_overlap(W.DEGENERATE_DIMS, edge, [[0, 1, 2]], W.tolerance(g, [[0, 1, 2]]))
    assert must.any() and not (must & ~got).any() and not (got & ~may).any()
    lo, hi = np.floor(g.min(0)).astype(int), np.floor(g.max(0)).astype(int)
    if name in ("repeated-vertex", "zero-length-edge", "collinear"):
        assert got.sum() < np.prod(hi - lo + 1) // 4         # far from the bounding box
    if name == "point":
        assert got.sum() == 1
    if name == "on-cell-planes":                             # a segment on the line x = 3, z = 5: the four cells around it, all along
        assert got.sum() == 4 * 9 and got[2:4, 1:10, 4:6].all()


# ---- the C++ loader ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


@pytest.fixture(scope="module")
def moving_sphere(tmp_path_factory):
    d = tmp_path_factory.mktemp("watertight")
    v, f = icosphere(11.0, (40.0, 42.0, 45.0), subdiv=1)
    data, cfg = str(d / "sphere_3D_data.txt"), str(d / "sphere_3D_config.txt")
    shape3d.write_mesh(data, [(v, f), (v * 0.9 + np.array([5.0, 4.0, 4.5]), f)])
    open(cfg, "w").write(CONFIG)
    return data, cfg, d


@pytest.mark.parametrize("time", [0.0, 0.0047])
@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("align", [True, False])
def test_cpp_loader_equals_the_twin(driver, moving_sphere, prec, align, time):
    data, cfg, d = moving_sphere
    dump = str(d / ("grid_%s_%d_%g.bin" % (prec, align, time)))
    args = [driver, data, str(d / "out"), cfg] + (["align"] if align else []) + ["--watertight", "--grid-only", dump] + \
           (["--grid-time", repr(time)] if time else []) + (["double"] if prec == "double" else [])
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout
    h = float(np.float32(0.001))
    nodes, sh = shape3d.load_shape3d(data, h, h, h, align=align, voxels="conservative")
    ref_nodes, _ = shape3d.load_shape3d(data, h, h, h, align=align)
    m = re.search(r"NODE_IN points = ([0-9.]+) of total", out)                  # (printed for the grid of time 0)
    assert float(m.group(1)) == float((nodes.type == grids.NODE_IN).sum()) != float((ref_nodes.type == grids.NODE_IN).sum())
    if time:
        sh.prepare(time)
        nodes = shape3d.nodes_of(sh, h, h, h, 1.0)
    g = _grid_dump(dump)
    assert np.array_equal(g["type"], nodes.type) and (nodes.type == grids.NODE_IN).any()
    assert not g["bc_vel"].any() and not g["bc_temp"].any() and not g["vx"].any()
    assert np.array_equal(g["T"], np.asarray(nodes.T, g["T"].dtype))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_voxel") / "mesh_voxel_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mesh_voxel_test.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("case", ["outside", "degenerate", "sphere-20", "tetra"])
def test_sanitized_builder_equals_the_twin(program, tmp_path, case):
    sh, g, idx, _ = W.gpu_case(case)
    src, dst = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    xyz, tri = capi.Solver._mesh_arrays(g, idx)
    with open(src, "wb") as f:
        np.array(list(sh.type.shape) + [len(xyz[0]), tri.size // 3], np.int32).tofile(f)
        for a in xyz + [tri]:
            a.tofile(f)
    r = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(dst, np.uint8).reshape(sh.type.shape)
    assert np.array_equal(got, sh.type), "%d cells differ" % int((got != sh.type).sum())


def test_sanitized_builder_refuses_a_coordinate_past_4096(program, tmp_path):
    src = str(tmp_path / "in.raw")
    with open(src, "wb") as f:
        np.array([8, 8, 8, 3, 1], np.int32).tofile(f)
        np.array([1, 2, 3, 1, 5000, 1, 1, 1, 2], np.float32).tofile(f)
        np.array([0, 1, 2], np.int32).tofile(f)
    r = subprocess.run([program, src, str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "4096" in r.stderr, r.stdout + r.stderr


# ---- the driver's word and the option ---------------------------------------------------------------------------------------------

def test_driver_refuses_watertight_for_a_shape2d_input(driver, tmp_path):
    data, cfg = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    r = subprocess.run([driver, data, str(tmp_path / "o"), cfg, "--watertight", "--grid-only", str(tmp_path / "g.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "--watertight: only in_fmt Shape3D inputs are meshes" in r.stderr and "Shape2D" in r.stderr
    assert "--watertight" in subprocess.run([driver], capture_output=True, text=True).stdout      # the usage line


def test_option_id_in_the_binding_and_the_header():
    assert capi.OPT_MESH_VOXELS == 8 and capi.MESH_VOXELS == {"reference": 0, "conservative": 1}
    enums = abi_decls.enumerators()
    assert enums["FS3D_OPT_MESH_VOXELS"] == capi.OPT_MESH_VOXELS
    ids = [v for k, v in enums.items() if k.startswith("FS3D_OPT_")]
    assert len(ids) == len(set(ids)), "two options share an id"
