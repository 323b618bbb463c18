"""GPU: the thin shell of the conservative Shape3D voxeliser (FS3D_OPT_MESH_SHELL = 1, k_geom_voxel_mesh<.., true>) against its twin
(shape3d.Shape3D(voxels="conservative", shell="cross")) byte for byte through fs3d_voxelize_shape3d_dev and
fs3d_update_nodes_shape3d, the wall velocities of its owners, a breathing run against the CPU oracle, x-slabs against a fresh upload
of the twin's nodes, the refusals and the unchanged default.  No tolerance appears: integers and bit patterns only."""
import ctypes as C
import json
import os
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
import mesh_slab_cases as MS  # noqa: E402
import test_gpu_moving as M  # noqa: E402
import thin_shell_cases as TS  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
import watertight_cases as W  # noqa: E402
from test_gpu_extrude import bare_context  # noqa: E402
from test_gpu_mesh import raw_update  # noqa: E402
from test_gpu_mesh_wall_velocity import differences, garbage  # noqa: E402
from test_gpu_slab_geometry import assert_same_context, params, tables  # noqa: E402
from cmc_fluid_solver_amd import capi, grids  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits


def child(*args):
    """`python tests/test_gpu_mesh_thin_shell.py <what>` in a fresh process in which torch opens the GPU first."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def by_name(nodes):
    return {name: getattr(nodes, name) for name in MC.NODE_ARRAYS}


# ---- 5. the kernel against the twin -------------------------------------------------------------------------------------------

def voxelize_all_cases():
    """every case of W.GPU_CASES in fp32 and fp64: fs3d_voxelize_shape3d_dev with the option into tensors that hold garbage, and
    fs3d_update_nodes_shape3d on a context that started from a box -- its bound_cells; once, option 0 set again: today's bytes"""
    import time
    import torch
    t0 = time.time()
    for case in W.GPU_CASES:
        thin, cons, g, idx, cell = TS.gpu_case(case)
        want, want0 = TS.nodes_of(thin), TS.nodes_of(cons)
        n = want.ncells
        for prec, dtype, td in (("f32", np.float32, torch.float32), ("f64", np.float64, torch.float64)):
            s = bare_context(want.shape, dtype, (thin.dx, thin.dy, thin.dz))
            by, va = garbage(torch, n, td)
            s.voxelize_shape3d_dev(g, idx, MC.BASE_T, *[t[:n] for t in by + va], voxels="conservative", shell="cross")
            rec = dict(case=case, prec=prec, dims=list(want.shape), seconds=round(time.time() - t0, 2), bound_cells=TS.counts(thin)[0], bad=differences(by_name(want), by + va, n),
                       closed=W.closed_report(by[0][:n].cpu().numpy().reshape(want.shape), cell) if cell else None)
            by, va = garbage(torch, n, td)                           # the option set back: the conservative shell, as before it existed
            s.voxelize_shape3d_dev(g, idx, MC.BASE_T, *[t[:n] for t in by + va], shell="box")
            rec["box_bad"] = differences(by_name(want0), by + va, n)
            s.close()
            start = grids.box(*want.shape)
            start.dx, start.dy, start.dz = want.dx, want.dy, want.dz
            u = capi.Solver(start, capi.fluid_params(dtype, *M.PARAMS), dtype)
            u.update_nodes_shape3d(g, idx, MC.BASE_T, voxels="conservative", shell="cross")
            rec["update_bound_cells"] = u.geometry_info()["bound_cells"]
            f = capi.Solver(want, capi.fluid_params(dtype, *M.PARAMS), dtype)
            iu, jf = u.geometry_info(), f.geometry_info()
            rec["update_tables_equal"] = [iu[k] for k in M.TABLE_KEYS] == [jf[k] for k in M.TABLE_KEYS]
            u.close(); f.close()
            print("CASE " + json.dumps(rec), flush=True)


@pytest.fixture(scope="module")
def voxelized(built):
    return [json.loads(l[5:]) for l in child("voxelize").splitlines() if l.startswith("CASE ")]


def one(voxelized, case, prec):
    mine = [r for r in voxelized if r["case"] == case and r["prec"] == prec]
    assert len(mine) == 1, "the child process did not reach %s %s" % (case, prec)
    return mine[0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", W.GPU_CASES)
def test_kernel_equals_the_twin(voxelized, case, prec):
    r = one(voxelized, case, prec)
    assert r["bad"] == [] and r["bound_cells"] == TS.PINS[case][0][1], r
    assert r["update_bound_cells"] == r["bound_cells"] and r["update_tables_equal"], r
    if r["closed"] is not None:
        W.assert_closed(r["closed"])
    if case == "ragged":
        assert r["dims"][2] % 4 != 0, r


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", W.GPU_CASES)
def test_option_zero_is_the_conservative_shell_as_before(voxelized, case, prec):
    assert one(voxelized, case, prec)["box_bad"] == []


@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact", "f32-auto"])
def test_update_from_the_mesh_equals_upload_of_the_thin_twin(built, mode):
    """the seven node arrays of fs3d_update_nodes_shape3d, through everything that reads them: tables, three time steps, the error"""
    dtype, kernel, f64_part = M.MODES[mode]
    sh, _ = W.sphere(80, (30, 38, 30))
    g1 = TS.nodes_of(sh)
    g = (sh.subframe(0.0)[0] * np.float32(0.9) + np.float32(3.0)).astype(np.float32)       # the same grid, a smaller sphere
    idx = sh.subframe(0.0)[1]
    g2 = TS.nodes_of(TS.thin(sh, g, idx))
    assert (g2.type == grids.NODE_IN).sum() > (TS.nodes_of(W.conservative(sh, g, idx)).type == grids.NODE_IN).sum()
    lay = M.seeded_layers(g2, dtype)
    a, b = M.make(g1, dtype, kernel, f64_part), M.make(g2, dtype, kernel, f64_part)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    nseg_a = a.update_nodes_shape3d(g, idx, MC.BASE_T, voxels="conservative", shell="cross")
    ia, ib = a.geometry_info(), b.geometry_info()
    assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
    assert nseg_a == b.num_segments and ia["bound_cells"] == int((g2.type == grids.NODE_BOUND).sum())
    for step in range(3):
        a.UpdateBoundaries(); b.UpdateBoundaries()
        a.TimeStep(dtype(M.DT), 2, 2, False); b.TimeStep(dtype(M.DT), 2, 2, False)
    assert a.eval_div_error(capi.LAYER_CUR) == b.eval_div_error(capi.LAYER_CUR)
    for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
        assert np.array_equal(bits(x), bits(y)), "field %d differs in %d cells" % (v, int((bits(x) != bits(y)).sum()))
    a.close(); b.close()


# ---- 6. wall velocities ---------------------------------------------------------------------------------------------------------

def wall_velocity_steps():
    """the translating sphere: the seven arrays of the _vel entry with the thin shell against the twin's, every step, fp32 and fp64"""
    import torch
    steps = TS.translating_grids()
    for prec, dtype, td in (("f32", np.float32, torch.float32), ("f64", np.float64, torch.float64)):
        s = bare_context(steps[0][0].shape, dtype, (steps[0][0].dx, steps[0][0].dy, steps[0][0].dz))
        for n_step, (thin, cons, g, vel, idx, own_t, own_c) in enumerate(steps):
            n = thin.ncells
            by, va = garbage(torch, n, td)
            s.voxelize_shape3d_vel_dev(g, vel, idx, MC.BASE_T, MC.BASE_T, *[t[:n] for t in by + va], voxels="conservative", shell="cross")
            print("STEP " + json.dumps(dict(prec=prec, step=n_step, bad=differences(by_name(thin), by + va, n))), flush=True)
        s.close()


@pytest.fixture(scope="module")
def wall_steps(built):
    return [json.loads(l[5:]) for l in child("walls").splitlines() if l.startswith("STEP ")]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_wall_velocities_of_the_thin_owners_equal_the_twin(wall_steps, prec):
    mine = [r for r in wall_steps if r["prec"] == prec]
    assert len(mine) == WV.RUN_STEPS and all(r["bad"] == [] for r in mine), mine


@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact"])
def test_update_with_velocities_equals_the_twin_and_owners_differ(built, mode):
    """fs3d_update_nodes_shape3d_vel with the option on the translating sphere: the context equals one that uploaded the twin's
    thin nodes (walls at WALL_SPEED), step after step; the thin owners are not the conservative run's"""
    dtype, kernel, f64_part = M.MODES[mode]
    steps = TS.translating_grids()
    a = M.make(steps[0][1], dtype, kernel, f64_part)
    a.set_option(capi.OPT_MESH_VOXELS, 1); a.set_option(capi.OPT_MESH_SHELL, 1)
    differing = 0
    for thin, cons, g, vel, idx, own_t, own_c in steps[:3]:
        a.update_nodes_shape3d_vel(g, vel, idx, MC.BASE_T, MC.BASE_T)
        b = M.make(thin, dtype, kernel, f64_part)
        ia, ib = a.geometry_info(), b.geometry_info()
        assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
        assert ia["bound_cells"] == int((thin.type == grids.NODE_BOUND).sum()) < int((cons.type == grids.NODE_BOUND).sum())
        for l in (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF, capi.LAYER_NEXT):
            b.upload_layer(l, a.download_layer(l))
        a.UpdateBoundaries(); b.UpdateBoundaries()
        assert a.TimeStep(dtype(WV.RUN_DT), 2, 1, True) == b.TimeStep(dtype(WV.RUN_DT), 2, 1, True)
        for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
            assert np.array_equal(bits(x), bits(y)), "field %d differs" % v
        b.close()
        wall = thin.type == grids.NODE_BOUND
        assert (np.asarray(thin.vx)[wall] > 0).all()          # every wall cell moves with the mesh
        differing += int((own_t[wall] != own_c[wall]).sum())
    assert differing > 0
    a.close()


# ---- 7. a breathing run ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact"])
def test_breathing_sphere_has_more_fluid_and_equals_the_oracle(built, mode):
    """the run of test_gpu_mesh_watertight.py::test_breathing_sphere_keeps_its_fluid_and_equals_the_oracle with the thin shell:
    at every step NODE_IN is larger than in the conservative run, the fields and the reported error equal the CPU oracle driven
    through the twin's thin grids, bit for bit."""
    dtype, kernel, f64_part = M.MODES[mode]
    O = M._oracle()
    sh, cell = W.sphere(80, (30, 38, 30))
    g0, idx = sh.subframe(0.0)
    centre = g0.mean(axis=0, dtype=np.float64)
    p = capi.fluid_params(dtype, *M.PARAMS)
    nodes0 = TS.nodes_of(TS.sphere(80, (30, 38, 30))[0])
    a = capi.Solver(nodes0, p, dtype)
    o = O.Oracle(nodes0, p, dtype)
    a.set_option(capi.OPT_SWEEP_KERNEL, kernel); a.set_option(capi.OPT_F64_PART, f64_part); a.set_option(capi.OPT_ERR_ORDER, 1)
    a.set_option(capi.OPT_MESH_VOXELS, 1); a.set_option(capi.OPT_MESH_SHELL, 1)
    dt = 0.01
    for n, s in enumerate((0.975, 0.95, 0.925, 0.9, 0.95, 1.0)):
        g = ((g0 - centre) * s + centre).astype(np.float32)
        nodes = TS.nodes_of(TS.thin(sh, g, idx))
        n_in, n_in_box = int((nodes.type == grids.NODE_IN).sum()), int((W.conservative(sh, g, idx).type == grids.NODE_IN).sum())
        a.update_nodes_shape3d(g, idx, MC.BASE_T)
        info = a.geometry_info()
        assert n_in > n_in_box > 0 and info["bound_cells"] == int((nodes.type == grids.NODE_BOUND).sum())
        a.UpdateBoundaries()
        ea = a.TimeStep(dtype(dt), 2, 1, True)
        assert np.isfinite(ea)
        o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in WV.oracle_arrays(nodes, dtype)])
        o._f("fs3d_oracle_create_segments")(o.h)
        o.update_boundaries()
        rc, eo = o.time_step(float(dtype(dt)), 2, 1, True)
        assert rc == 0 and eo == ea, (n, eo, ea)
        M.clear_oracle(o, nodes.type == grids.NODE_OUT, MC.BASE_T)
        a.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); a.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        fa = a.download_layer(capi.LAYER_CUR)
        for v, y in enumerate(o.get_layer_fields(O.L_CUR)):
            assert np.array_equal(bits(fa[v]), bits(np.ascontiguousarray(y, dtype))), "step %d field %d differs from the oracle" % (n, v)
    a.close(); o.close()


# ---- 8. x-slabs --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_slab_update_with_the_thin_shell_equals_a_fresh_upload(built, nranks, dtype, monkeypatch):
    """sphere-20 on 28 x 35 x 28, 2 and 3 ranks, both slab entries: the tables equal those of a fresh slab context that uploaded
    the twin's thin nodes of the global grid"""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    thin, cons, g, idx, _ = TS.gpu_case("sphere-20")
    idx = np.asarray(idx).reshape(-1, 3)
    vel = (WV.velocities(g) * np.float32(2.0 ** -10)).astype(np.float32)
    plain = MS.Case(TS.nodes_of(thin), np.array(g, np.float32), idx, "conservative")
    moving = MS.Case(WV.nodes_of(TS.thin(thin, g, idx, vel)), np.array(g, np.float32), idx, "conservative", vel, WV.WALL_T)
    for case in (plain, moving):
        start = case.start()
        for xr in MS.ranges(case.want.dimx, nranks):
            s = capi.Solver(start, params(dtype), dtype, x_range=xr)
            s.set_option(capi.OPT_MESH_SHELL, 1)
            nseg = case.update(s)
            f = capi.Solver(case.want, params(dtype), dtype, x_range=xr)
            print(nranks, xr, tables(s))
            assert nseg == f.num_segments
            assert_same_context(s, f, "planes %s of %d ranks" % (xr, nranks))
            s.close(); f.close()


# ---- 9. refusals and the default ---------------------------------------------------------------------------------------------------

def test_option_values_and_the_refusal_without_the_conservative_voxelisation(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_EXACT)
    xyz, tri = s._mesh_arrays(g, idx)
    nv, nt = len(xyz[0]), tri.size // 3
    for bad in (2, -1):
        assert s.lib.fs3d_set_option(s.h, capi.OPT_MESH_SHELL, bad) == capi.ERR_INVALID
        assert s.lib.fs3d_set_option(s.h, capi.OPT_MESH_VOXELS, 2) == capi.ERR_INVALID
    with pytest.raises(ValueError):
        s.update_nodes_shape3d(g, idx, MC.BASE_T, shell="thin")
    s.set_option(capi.OPT_MESH_SHELL, 1)                 # FS3D_OPT_MESH_VOXELS is 0
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]
    st, msg = raw_update(s, xyz, nv, tri, nt)
    assert st == capi.ERR_INVALID and "FS3D_OPT_MESH_SHELL" in msg and "conservative" in msg, (st, msg)
    one_ = np.zeros(8, np.uint8)                         # never read: refused before anything is launched
    args = [capi._p(a) for a in xyz] + [nv, capi._p(tri), nt, 1.0] + [capi._p(one_)] * 7
    assert s.lib.fs3d_voxelize_shape3d_dev(s.h, *args) == capi.ERR_INVALID and b"FS3D_OPT_MESH_SHELL" in s.lib.fs3d_last_error(s.h)
    nseg = (C.c_int * 3)()
    assert s.lib.fs3d_update_nodes_shape3d_slab(s.h, *[capi._p(a) for a in xyz], nv, capi._p(tri), nt, 1.0, nseg) == capi.ERR_INVALID
    after = s.geometry_info()                            # refused before anything was touched: same tables, nothing counted, the context steps on
    assert after == before and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    s.set_option(capi.OPT_MESH_VOXELS, 1)                # and the same call with the conservative voxelisation goes through
    st, msg = raw_update(s, xyz, nv, tri, nt)
    assert st == capi.OK, msg
    thin = TS.thin(sh, g, idx)
    assert s.geometry_info()["bound_cells"] == TS.counts(thin)[0] < TS.counts(W.conservative(sh, g, idx))[0]
    s.set_option(capi.OPT_MESH_SHELL, 0)                 # the default again: the conservative shell
    assert raw_update(s, xyz, nv, tri, nt)[0] == capi.OK
    assert s.geometry_info()["bound_cells"] == TS.counts(W.conservative(sh, g, idx))[0]
    s.close()


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "voxelize":
        voxelize_all_cases()
    if sys.argv[1] == "walls":
        wall_velocity_steps()
