"""GPU: walls of a Shape3D mesh that carry the mesh's velocity -- fs3d_voxelize_shape3d_vel_dev (k_geom_voxel_mesh<true>,
k_geom_mesh_nodes_vel) against the twin byte for byte, the zero guarantee against fs3d_voxelize_shape3d_dev,
fs3d_update_nodes_shape3d_vel against an upload of the twin's nodes bit for bit, the translating sphere against the CPU oracle,
the refusals, the allocation contract and the driver's --wall-velocity.  No tolerance appears: integers and bit patterns only."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:          # run as a script (the child process below)
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import mesh_cases as MC  # noqa: E402
import test_gpu_moving as M  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
import watertight_cases as W  # noqa: E402
from test_gpu_extrude import bare_context  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape3d  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits
ZERO_CASES = ("sphere-20", "ragged", "degenerate")


def child(*args):
    """`python tests/test_gpu_mesh_wall_velocity.py <what>` in a fresh process in which torch opens the GPU first."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


# ---- 6, 7. the kernels against the twin, and the zero guarantee -----------------------------------------------------------------

def garbage(torch, n, td):
    by = [torch.full((n + 4,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
    va = [torch.full((n + 4,), float("nan"), dtype=td, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    return by, va


def differences(want, tensors, n):
    """names of the arrays that differ from `want` (numpy arrays by name) in a byte, or whose guard elements were written"""
    bad = []
    for name, t in zip(MC.NODE_ARRAYS, tensors):
        got = t.cpu().numpy()
        exp = np.ascontiguousarray(want[name], got.dtype).reshape(-1)
        if not np.array_equal(got[:n].view(np.uint8), exp.view(np.uint8)):
            bad.append("%s: %d cells" % (name, int((got[:n] != exp).sum())))
        if not (np.isnan(got[n:]).all() if got.dtype.kind == "f" else (got[n:] == 0xAB).all()):
            bad.append(name + "-outside")
    return bad


def voxelize_all_cases():
    import torch
    for case in WV.GPU_CASES:
        for reverse in (False, True):
            nodes, g, vel, idx = WV.expected(case, reverse)
            want = {name: getattr(nodes, name) for name in MC.NODE_ARRAYS}
            n = nodes.ncells
            for prec, dtype, td in (("f32", np.float32, torch.float32), ("f64", np.float64, torch.float64)):
                s = bare_context(nodes.shape, dtype, (nodes.dx, nodes.dy, nodes.dz))
                by, va = garbage(torch, n, td)
                s.voxelize_shape3d_vel_dev(g, vel, idx, MC.BASE_T, WV.WALL_T, *[t[:n] for t in by + va], voxels="conservative")
                wall = nodes.type == grids.NODE_BOUND
                rec = dict(case=case, prec=prec, reverse=reverse, dims=list(nodes.shape), bound_cells=int(wall.sum()),
                           moving_cells=int((np.asarray(nodes.vx)[wall] != 0).sum()), bad=differences(want, by + va, n))
                if case in ZERO_CASES and not reverse:                # zero velocities, wallT = 0: the existing entry's arrays
                    by0, va0 = garbage(torch, n, td)
                    s.voxelize_shape3d_dev(g, idx, MC.BASE_T, *[t[:n] for t in by0 + va0])
                    by1, va1 = garbage(torch, n, td)
                    s.voxelize_shape3d_vel_dev(g, np.zeros_like(vel), idx, MC.BASE_T, 0.0, *[t[:n] for t in by1 + va1])
                    rec["zero_bad"] = differences({name: t.cpu().numpy()[:n] for name, t in zip(MC.NODE_ARRAYS, by0 + va0)}, by1 + va1, n)
                s.close()
                print("CASE " + json.dumps(rec), flush=True)


@pytest.fixture(scope="module")
def voxelized(built):
    return [json.loads(l[5:]) for l in child("voxelize").splitlines() if l.startswith("CASE ")]


def one(voxelized, case, prec, reverse=False):
    mine = [r for r in voxelized if r["case"] == case and r["prec"] == prec and r["reverse"] == reverse]
    assert len(mine) == 1, "the child process did not reach %s %s" % (case, prec)
    return mine[0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("reverse", [False, True], ids=["listed", "reversed"])
@pytest.mark.parametrize("case", WV.GPU_CASES)
def test_kernels_equal_the_twin(voxelized, case, reverse, prec):
    r = one(voxelized, case, prec, reverse)
    assert r["bad"] == [] and r["bound_cells"] > 0 and r["moving_cells"] > r["bound_cells"] // 2, r
    if case == "ragged":
        assert r["dims"][2] % 4 != 0, r


def test_a_reversed_list_changes_the_expected_bytes():
    a, b = WV.expected("sphere-20")[0], WV.expected("sphere-20", True)[0]
    assert np.array_equal(a.type, b.type) and not np.array_equal(a.vx, b.vx)      # (else the reversed cases would prove nothing)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", ZERO_CASES)
def test_zero_velocities_and_wall_temperature_zero_equal_the_existing_entry(voxelized, case, prec):
    assert one(voxelized, case, prec)["zero_bad"] == []


# ---- 8. a context updated from the mesh against a fresh upload of the twin's nodes -----------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact", "f32-auto"])
def test_update_with_velocities_equals_upload_of_the_twin(built, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    sh, _ = W.sphere(80, (30, 38, 30))
    g1 = MC.nodes_of(sh)
    g = (sh.subframe(0.0)[0] * np.float32(0.9) + np.float32(3.0)).astype(np.float32)       # the same grid, a smaller sphere
    idx = np.asarray(sh.subframe(0.0)[1]).reshape(-1, 3)
    vel = (WV.velocities(g) * np.float32(2.0 ** -10)).astype(np.float32)                    # non-uniform, below 0.2 in magnitude
    g2 = WV.nodes_of(WV.built(sh, g, idx, vel))
    assert np.abs(np.asarray(g2.vx)[g2.type == grids.NODE_BOUND]).max() > 0.01 and (g2.type == grids.NODE_IN).any()
    lay = M.seeded_layers(g2, dtype)
    a, b = M.make(g1, dtype, kernel, f64_part), M.make(g2, dtype, kernel, f64_part)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    nseg_a = a.update_nodes_shape3d_vel(g, vel, idx, MC.BASE_T, WV.WALL_T, voxels="conservative")
    ia, ib = a.geometry_info(), b.geometry_info()
    print("mesh:  ", ia, "\nupload:", ib)
    assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
    assert nseg_a == b.num_segments and ia["segments_z"] > 0
    for step in range(3):
        a.UpdateBoundaries(); b.UpdateBoundaries()
        a.TimeStep(dtype(M.DT), 2, 2, False); b.TimeStep(dtype(M.DT), 2, 2, False)
    assert a.eval_div_error(capi.LAYER_CUR) == b.eval_div_error(capi.LAYER_CUR)
    assert a.last_sweep_kernels() == b.last_sweep_kernels()
    for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
        assert np.array_equal(bits(x), bits(y)), "field %d differs in %d cells" % (v, int((bits(x) != bits(y)).sum()))
    a.close(); b.close()


# ---- 9. the translating sphere ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact"])
def test_translating_sphere_equals_the_oracle_and_carries_its_fluid(built, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    O = M._oracle()
    steps = WV.translating_grids()
    params = capi.fluid_params(dtype, *M.PARAMS)
    a = capi.Solver(steps[0][0], params, dtype)
    o = O.Oracle(steps[0][0], params, dtype)
    a.set_option(capi.OPT_SWEEP_KERNEL, kernel); a.set_option(capi.OPT_F64_PART, f64_part); a.set_option(capi.OPT_ERR_ORDER, 1)
    a.set_option(capi.OPT_MESH_VOXELS, 1)
    for n, (nodes, g, vel, idx) in enumerate(steps):
        a.update_nodes_shape3d_vel(g, vel, idx, MC.BASE_T, MC.BASE_T)
        assert a.geometry_info()["bound_cells"] == int((nodes.type == grids.NODE_BOUND).sum())
        a.UpdateBoundaries()
        ea = a.TimeStep(dtype(WV.RUN_DT), WV.RUN_GL[0], WV.RUN_GL[1], True)
        rc, eo = WV.oracle_step(O, o, nodes, dtype, M.clear_oracle)
        assert rc == 0 and eo == ea and ea < 0.01, (n, eo, ea)
        a.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); a.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        fa = a.download_layer(capi.LAYER_CUR)
        for v, y in enumerate(o.get_layer_fields(O.L_CUR)):
            assert np.array_equal(bits(fa[v]), bits(np.ascontiguousarray(y, dtype))), "step %d field %d differs from the oracle" % (n, v)
    mean_u = float(np.asarray(fa[0], np.float64)[steps[-1][0].type == grids.NODE_IN].mean())
    print("mean u over NODE_IN", mean_u)
    assert mean_u >= 0.9 * WV.WALL_SPEED
    a.close(); o.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------

def raw_update_vel(s, xyz, w, nvert, tri, ntri, wallT=WV.WALL_T):
    nseg = (C.c_int * 3)()
    st = s.lib.fs3d_update_nodes_shape3d_vel(s.h, *[capi._p(a) for a in list(xyz) + list(w)], nvert, capi._p(tri), ntri, 1.0, wallT, nseg)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


def test_refusals_leave_the_context_as_it_was(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_EXACT)
    xyz, tri = s._mesh_arrays(g, idx)
    w = s._mesh_velocities(WV.velocities(g) * np.float32(2.0 ** -10), len(xyz[0]))
    nv, nt = len(xyz[0]), tri.size // 3
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]
    st, msg = raw_update_vel(s, xyz, w, nv, tri, nt)                     # FS3D_OPT_MESH_VOXELS is 0
    assert st == capi.ERR_INVALID and "conservative" in msg, (st, msg)
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    for bad_value in (np.nan, np.inf, -np.inf):
        w2 = [a.copy() for a in w]; w2[2][5] = bad_value
        st, msg = raw_update_vel(s, xyz, w2, nv, tri, nt)
        assert st == capi.ERR_INVALID and "velocity" in msg and "finite" in msg, (bad_value, st, msg)
    for bad_value in (np.nan, np.inf):
        st, msg = raw_update_vel(s, xyz, w, nv, tri, nt, wallT=bad_value)
        assert st == capi.ERR_INVALID and "temperature" in msg, (bad_value, st, msg)
    for hole in range(3):                                                # NULL, each velocity array in turn
        st, msg = raw_update_vel(s, xyz, [None if q == hole else a for q, a in enumerate(w)], nv, tri, nt)
        assert st == capi.ERR_INVALID and "NULL" in msg, (hole, st, msg)
    one_ = np.zeros(8, np.uint8)                                         # never read: refused before anything is launched
    args = [capi._p(a) for a in xyz + [w[0], None, w[2]]] + [nv, capi._p(tri), nt, 1.0, 0.0] + [capi._p(one_)] * 7
    assert s.lib.fs3d_voxelize_shape3d_vel_dev(s.h, *args) == capi.ERR_INVALID
    after = s.geometry_info()                    # refused before anything was touched: same tables, nothing counted, the context steps on
    assert after == before and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    st, msg = raw_update_vel(s, xyz, w, nv, tri, nt)                     # and the same call with nothing wrong goes through
    assert st == capi.OK, msg
    assert s.profiler_events()["CreateSegments"][1] == n_before + 1
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    s.close()


def test_a_slab_context_is_unsupported(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = capi.Solver(MC.nodes_of(sh), capi.fluid_params(np.float32, *M.PARAMS), np.float32, x_range=(0, 16))
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    xyz, tri = s._mesh_arrays(g, idx)
    w = s._mesh_velocities(np.zeros_like(g), len(xyz[0]))
    st, msg = raw_update_vel(s, xyz, w, len(xyz[0]), tri, tri.size // 3)
    assert st == capi.ERR_UNSUPPORTED and "single context" in msg
    one_ = np.zeros(8, np.uint8)
    args = [capi._p(a) for a in xyz + w] + [len(xyz[0]), capi._p(tri), tri.size // 3, 1.0, 0.0] + [capi._p(one_)] * 7
    assert s.lib.fs3d_voxelize_shape3d_vel_dev(s.h, *args) == capi.ERR_UNSUPPORTED and b"single context" in s.lib.fs3d_last_error(s.h)
    s.UpdateBoundaries()                 # refused before anything was touched: the slab keeps its geometry
    s.close()


# ---- 11. allocations -----------------------------------------------------------------------------------------------------------------

def test_steady_state_allocates_nothing(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_AUTO)
    tw, _ = MC.twin("sphere_3D")
    s.enable_timing(True)
    allocs = []
    for r in range(6):
        t = 0.003 * r
        s.update_nodes_shape3d_vel(tw.subframe(t)[0], tw.subframe_velocity(t, "motion"), tw.subframe(t)[1], MC.BASE_T, WV.WALL_T, voxels="conservative")
        assert s.last_update_device_ms() > 0
        allocs.append(s.geometry_info()["device_allocs_and_frees"])
    print("allocs + frees after each update:", allocs)
    assert allocs[0] > 0 and all(x == allocs[0] for x in allocs[1:])
    s.close()


def test_the_existing_entry_allocates_what_it_did(built):
    """the owner array belongs to the new entries alone: a context that only ever calls fs3d_update_nodes_shape3d makes one
    allocation fewer than one that calls fs3d_update_nodes_shape3d_vel"""
    sh, g, idx, _ = MC.load_case("sphere-t0")
    counts = []
    for vel in (False, True):
        s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_AUTO)
        if vel:
            s.update_nodes_shape3d_vel(g, np.zeros_like(g), idx, MC.BASE_T, 0.0, voxels="conservative")
        else:
            s.update_nodes_shape3d(g, idx, MC.BASE_T, voxels="conservative")
        counts.append(s.geometry_info()["device_allocs_and_frees"])
        s.close()
    assert counts[1] == counts[0] + 1, counts


# ---- 12. the driver ------------------------------------------------------------------------------------------------------------------

def test_driver_wall_velocity_equals_host_voxels_and_differs_from_walls_at_rest(built, tmp_path):
    """sphere_3D moves 1 mm in x and 0.5 mm in z per frame of 1/75 s: 0.075 m/s.  (On the CPU oracle, through the twin's grids, the
    reported error of this run stays below 0.01 with moving walls: the driver would stop with "Error is too big!" otherwise.)"""
    driver = B.build_driver()
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    walls = ["--watertight", "--wall-velocity", "motion", "--wall-temperature", "1"]
    outs = {}
    for word, extra in (("device", ["moving-mesh"] + walls), ("host", ["moving-mesh", "--host-voxels"] + walls), ("rest", ["moving-mesh", "--watertight"])):
        prefix = str(tmp_path / word)
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + extra, check=True, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
        errs = re.findall(r"err = ([0-9.]+),", r.stdout)
        outs[word] = (errs, open(prefix + "_res.nc", "rb").read())
    print(outs["device"][0], outs["rest"][0])
    assert len(outs["device"][0]) in (7, 8) and outs["device"][0] == outs["host"][0]
    assert all(float(e) < 0.01 for e in outs["device"][0])
    assert len(outs["device"][1]) > 1000 and outs["device"][1] == outs["host"][1]
    assert len(outs["rest"][1]) == len(outs["device"][1]) and outs["rest"][1] != outs["device"][1]


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "voxelize":
        voxelize_all_cases()
