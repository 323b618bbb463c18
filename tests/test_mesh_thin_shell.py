"""CPU: the thin (6-separating) shell of the conservative Shape3D voxeliser (voxels="conservative", shell="cross",
fs3d_run --watertight --thin-shell, FS3D_OPT_MESH_SHELL).  The twin (cmc_fluid_solver_amd/shape3d.py) is held to closedness on every
sphere of tests/watertight_cases.py, to pinned cell counts and to a float64 separating-axis test of the centre cross that shares
nothing with its loops (tests/thin_shell_cases.py); the C++ loader (host/Shape3D.h) is held to the twin cell for cell through the
driver and through a stand-alone program built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_decls
import thin_shell_cases as TS
import watertight_cases as W
from test_shape3d import CONFIG, _grid_dump, icosphere
from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, grids, shape3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. closedness, subset, thinness --------------------------------------------------------------------------------------------

def held_to_the_conservative_shell(thin, cons, cell):
    """closed; a subset of the conservative shell; fewer than 2/3 of its cells; every conservative NODE_IN cell still NODE_IN
    -> the ratio of the two shells"""
    W.assert_closed(W.closed_report(thin.type, cell))
    bt, bc = thin.type == grids.NODE_BOUND, cons.type == grids.NODE_BOUND
    assert not (bt & ~bc).any()
    assert 3 * int(bt.sum()) < 2 * int(bc.sum()), (int(bt.sum()), int(bc.sum()))
    assert (thin.type[cons.type == grids.NODE_IN] == grids.NODE_IN).all()
    return bt.sum() / bc.sum(), (thin.type == grids.NODE_IN).sum() / (cons.type == grids.NODE_IN).sum()


@pytest.mark.parametrize("faces", [20, 80, 320])
def test_thin_shell_is_closed_on_every_sphere(faces):
    """r = s (30, 38, 30), s = 0.5 .. 1.0 in 21 steps (the default rasteriser leaks on 18 of the 63)"""
    seen = [held_to_the_conservative_shell(*TS.sphere(faces, tuple(s * x for x in (30, 38, 30)))) for s in W.SCALES]
    print(faces, "faces: shell ratio %.3f .. %.3f, NODE_IN ratio %.3f .. %.3f" %
          (min(r for r, _ in seen), max(r for r, _ in seen), min(f for _, f in seen), max(f for _, f in seen)))


@pytest.mark.parametrize("faces,r,dims", W.SINGLE)
def test_single_leaking_spheres_are_closed_with_the_thin_shell(faces, r, dims):
    thin, cons, cell = TS.sphere(faces, r)
    assert thin.type.shape == dims
    held_to_the_conservative_shell(thin, cons, cell)


# ---- 2. pins of the rule ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", W.GPU_CASES)
def test_cell_counts_of_the_rule(case):
    thin, cons, g, idx, cell = TS.gpu_case(case)
    (bound_c, bound_t), fluid = TS.PINS[case]
    print(case, TS.counts(cons), "->", TS.counts(thin))
    assert TS.counts(cons)[0] == bound_c and TS.counts(thin)[0] == bound_t
    if fluid is not None:
        assert (TS.counts(cons)[1], TS.counts(thin)[1]) == fluid
    assert not ((thin.type == grids.NODE_BOUND) & (cons.type != grids.NODE_BOUND)).any()
    if case.startswith("degenerate"):                         # degenerate triangles keep the conservative treatment
        assert np.array_equal(thin.type, cons.type) and np.array_equal(thin.owner, cons.owner)


def test_owner_is_the_smallest_triangle_whose_thin_test_sets_the_cell():
    """painted independently, one single-triangle thin grid per triangle in descending index order; it differs from the
    conservative owner on cells that stay walls (a triangle of smaller index touched the box, not the centre cross)"""
    thin, cons, g, idx, _ = TS.gpu_case("sphere-20")
    idx = np.asarray(idx).reshape(-1, 3)
    own = np.full(thin.type.shape, shape3d.NO_OWNER, np.int64)
    for t in range(len(idx) - 1, -1, -1):
        own[TS.thin(thin, g, idx[t:t + 1]).type == grids.NODE_BOUND] = t
    assert np.array_equal(own, thin.owner)
    wall = thin.type == grids.NODE_BOUND
    assert (thin.owner[wall] >= cons.owner[wall]).all() and (thin.owner[wall] != cons.owner[wall]).any()


# ---- 3. the float64 restatement ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated():
    return {c: TS.restatement(*(TS.gpu_case(c)[i] for i in (0, 2, 3))) for c in TS.RESTATED}


@pytest.mark.parametrize("case", TS.RESTATED)
def test_twin_equals_the_float64_centre_cross_test(restated, case):
    shell, missing, extra, free = restated[case]
    print(case, "shell %d cells, %d missing, %d extra, %d free" % (shell, missing, extra, free))
    assert shell == TS.PINS[case][0][1] and missing == 0 and extra == 0
    assert free < 0.01 * shell


def test_the_restatement_tells_a_thick_shell_from_a_thin_one():
    """(else it would prove nothing) the conservative grid held to the thin restatement has extra cells, about 0.45 of them"""
    thin, cons, g, idx, _ = TS.gpu_case("sphere-20")
    shell, missing, extra, free = TS.restatement(cons, g, idx)
    assert missing == 0 and extra == shell - TS.PINS["sphere-20"][0][1]


# ---- keyword and refusals -----------------------------------------------------------------------------------------------------------

def test_keyword_defaults_and_refusals():
    txt, _ = W.sphere_text(20, (15, 19, 15))
    load = lambda **kw: shape3d.load_shape3d(txt, W.H, W.H, W.H, align=False, is_text=True, **kw)
    a, sa = load(voxels="conservative")
    b, sb = load(voxels="conservative", shell="box")
    c, sc = load(voxels="conservative", shell="cross")
    assert np.array_equal(a.type, b.type) and sa.shell == sb.shell == "box" and sc.shell == "cross"
    assert np.array_equal(c.type, TS.gpu_case("sphere-20")[0].type) and not np.array_equal(a.type, c.type)
    assert (c.T[c.type == grids.NODE_BOUND] == 0).all() and (c.T[c.type != grids.NODE_BOUND] == 1).all() and not c.vx.any()
    for kw in (dict(shell="cross"), dict(voxels="reference", shell="cross"), dict(voxels="conservative", shell="thin"), dict(voxels="thin")):
        with pytest.raises(ValueError):
            load(**kw)
    sc.prepare(0.0)                                           # a prepared twin keeps its shell
    assert np.array_equal(sc.type, c.type)


def test_option_id_in_the_binding_and_the_header():
    assert capi.OPT_MESH_SHELL == 11 and capi.MESH_SHELL == {"box": 0, "cross": 1}
    assert capi.MESH_VOXELS == {"reference": 0, "conservative": 1}
    enums = abi_decls.enumerators()
    assert enums["FS3D_OPT_MESH_SHELL"] == capi.OPT_MESH_SHELL
    ids = [v for k, v in enums.items() if k.startswith("FS3D_OPT_")]
    assert len(ids) == len(set(ids)), "two options share an id"


# ---- 4. the C++ loader ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


@pytest.fixture(scope="module")
def moving_sphere(tmp_path_factory):
    d = tmp_path_factory.mktemp("thin_shell")
    v, f = icosphere(11.0, (40.0, 42.0, 45.0), subdiv=1)
    data, cfg = str(d / "sphere_3D_data.txt"), str(d / "sphere_3D_config.txt")
    shape3d.write_mesh(data, [(v, f), (v * 0.9 + np.array([5.0, 4.0, 4.5]), f)])
    open(cfg, "w").write(CONFIG)
    return data, cfg, d


@pytest.mark.parametrize("prec", ["float", "double"])
@pytest.mark.parametrize("align", [True, False])
def test_cpp_loader_equals_the_twin(driver, moving_sphere, prec, align):
    data, cfg, d = moving_sphere
    time = 0.0047
    dump = str(d / ("grid_%s_%d.bin" % (prec, align)))
    args = [driver, data, str(d / "out"), cfg] + (["align"] if align else []) + ["--watertight", "--thin-shell", "--grid-only", dump,
            "--grid-time", repr(time)] + (["double"] if prec == "double" else [])
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout
    h = float(np.float32(0.001))
    nodes, sh = shape3d.load_shape3d(data, h, h, h, align=align, voxels="conservative", shell="cross")
    cons, _ = shape3d.load_shape3d(data, h, h, h, align=align, voxels="conservative")
    m = re.search(r"NODE_IN points = ([0-9.]+) of total", out)                  # (printed for the grid of time 0)
    assert float(m.group(1)) == float((nodes.type == grids.NODE_IN).sum()) > float((cons.type == grids.NODE_IN).sum())
    sh.prepare(time)
    nodes = shape3d.nodes_of(sh, h, h, h, 1.0)
    g = _grid_dump(dump)
    assert np.array_equal(g["type"], nodes.type) and (nodes.type == grids.NODE_IN).any()
    assert not g["bc_vel"].any() and not g["bc_temp"].any() and not g["vx"].any()
    assert np.array_equal(g["T"], np.asarray(nodes.T, g["T"].dtype))


def test_cpp_loader_owners_carry_the_wall_velocity_of_the_twin(driver, moving_sphere):
    """--wall-velocity motion with the thin shell: the owner is the thin test's, so the velocities equal the twin's bit for bit"""
    data, cfg, d = moving_sphere
    time = 0.0047
    dump = str(d / "grid_vel.bin")
    subprocess.run([driver, data, str(d / "out"), cfg, "--watertight", "--thin-shell", "--wall-velocity", "motion", "--grid-only", dump,
                    "--grid-time", repr(time)], check=True, capture_output=True, text=True)
    h = float(np.float32(0.001))
    nodes, sh = shape3d.load_shape3d(data, h, h, h, align=False, voxels="conservative", shell="cross", wall_velocity="motion", time=time)
    _, cons = shape3d.load_shape3d(data, h, h, h, align=False, voxels="conservative", wall_velocity="motion", time=time)
    g = _grid_dump(dump)
    assert np.array_equal(g["type"], nodes.type)
    for name in ("vx", "vy", "vz"):
        want = np.asarray(getattr(nodes, name), np.float32)
        assert np.array_equal(g[name].view(np.uint32), want.view(np.uint32)), name
    wall = sh.type == grids.NODE_BOUND
    assert g["vx"][wall].any() and (sh.owner[wall] != cons.owner[wall]).any()


def test_driver_refuses_thin_shell_without_watertight(driver, moving_sphere):
    data, cfg, d = moving_sphere
    r = subprocess.run([driver, data, str(d / "o"), cfg, "--thin-shell", "--grid-only", str(d / "g.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "--thin-shell: needs --watertight" in r.stderr
    assert "[--watertight [--thin-shell]" in subprocess.run([driver], capture_output=True, text=True).stdout      # the usage line


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_thin_shell") / "mesh_thin_shell_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mesh_thin_shell_test.cpp"), "-o", exe])
    return exe


def run_program(program, tmp_path, sh, g, idx, voxels, shell):
    src, dst = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    xyz, tri = capi.Solver._mesh_arrays(g, idx)
    with open(src, "wb") as f:
        np.array(list(sh.type.shape) + [len(xyz[0]), tri.size // 3], np.int32).tofile(f)
        for a in xyz + [tri]:
            a.tofile(f)
    r = subprocess.run([program, src, dst, str(voxels), str(shell)], capture_output=True, text=True, timeout=120)
    return r, dst


@pytest.mark.parametrize("case", ["outside", "degenerate", "sphere-20", "tetra", "ragged"])
def test_sanitized_builder_equals_the_twin(program, tmp_path, case):
    thin, cons, g, idx, _ = TS.gpu_case(case)
    for shell, sh in ((1, thin), (0, cons)):
        r, dst = run_program(program, tmp_path, sh, g, idx, 1, shell)
        assert r.returncode == 0, r.stdout + r.stderr
        n = sh.type.size
        got = np.fromfile(dst, np.uint8, n).reshape(sh.type.shape)
        own = np.fromfile(dst, np.int32, offset=n).reshape(sh.type.shape)
        assert np.array_equal(got, sh.type), "shell %d: %d cells differ" % (shell, int((got != sh.type).sum()))
        assert np.array_equal(own, sh.owner), "shell %d: %d owners differ" % (shell, int((own != sh.owner).sum()))


def test_sanitized_builder_refuses_bad_modes(program, tmp_path):
    thin, cons, g, idx, _ = TS.gpu_case("outside")
    for voxels, shell, word in ((0, 1, "conservative"), (1, 2, "shell is 0"), (1, -1, "shell is 0")):
        r, _ = run_program(program, tmp_path, thin, g, idx, voxels, shell)
        assert r.returncode == 3 and word in r.stderr, (voxels, shell, r.stdout + r.stderr)
