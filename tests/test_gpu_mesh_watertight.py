"""GPU: the conservative Shape3D voxeliser (FS3D_OPT_MESH_VOXELS = 1, k_geom_voxel_mesh) against its twin
(shape3d.Shape3D(voxels="conservative")) byte for byte, closedness of the device grid where the default leaks, the option's
default, fs3d_update_nodes_shape3d against an upload of the twin's nodes bit for bit, a breathing run against the CPU oracle, the
refusals, the allocation contract and the driver's --watertight.  No tolerance appears: integers and bit patterns only."""
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
import watertight_cases as W  # noqa: E402
from test_gpu_extrude import bare_context  # noqa: E402
from test_gpu_mesh import raw_update  # noqa: E402
from test_shape3d import CONFIG, icosphere  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape3d  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits
LEAKING = ("sphere-20", "sphere-80")


def child(*args):
    """`python tests/test_gpu_mesh_watertight.py <what>` in a fresh process in which torch opens the GPU first."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def nodes_of(sh):
    return shape3d.nodes_of(sh, sh.dx, sh.dy, sh.dz, MC.BASE_T)


# ---- 1. the kernel against the twin -------------------------------------------------------------------------------------------

def voxelize_one(s, torch, td, want, g, idx, voxels):
    """the seven arrays through voxelize_shape3d_dev into tensors that hold garbage before the call -> (differences, type array)"""
    n = want.ncells
    by = [torch.full((n + 4,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
    va = [torch.full((n + 4,), float("nan"), dtype=td, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    s.voxelize_shape3d_dev(g, idx, MC.BASE_T, *[t[:n] for t in by + va], voxels=voxels)
    bad = []
    for name, t in zip(MC.NODE_ARRAYS, by + va):
        got = t.cpu().numpy()
        exp = np.ascontiguousarray(getattr(want, name), got.dtype).reshape(-1)
        if not np.array_equal(got[:n].view(np.uint8), exp.view(np.uint8)):
            bad.append("%s: %d cells" % (name, int((got[:n] != exp).sum())))
        if not (np.isnan(got[n:]).all() if got.dtype.kind == "f" else (got[n:] == 0xAB).all()):
            bad.append(name + "-outside")
    return bad, by[0][:n].cpu().numpy().reshape(want.shape)


def voxelize_all_cases():
    import torch
    for case in W.GPU_CASES:
        sh, g, idx, cell = W.gpu_case(case)
        want = nodes_of(sh)
        for prec, dtype, td in (("f32", np.float32, torch.float32), ("f64", np.float64, torch.float64)):
            s = bare_context(want.shape, dtype, (sh.dx, sh.dy, sh.dz))
            bad, ty = voxelize_one(s, torch, td, want, g, idx, "conservative")
            rec = dict(case=case, prec=prec, dims=list(want.shape), bound_cells=int((want.type == grids.NODE_BOUND).sum()), bad=bad,
                       closed=W.closed_report(ty, cell) if cell else None)
            if case == "sphere-80" and prec == "f32":              # option 0, set explicitly: today's path, the reference-mode twin
                ref = nodes_of(W.sphere(80, (30, 38, 30), "reference")[0])
                rec["option0_bad"], ty0 = voxelize_one(s, torch, td, ref, g, idx, "reference")
                rec["option0_fluid_cells"] = int((ty0 == grids.NODE_IN).sum())
            s.close()
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
    assert r["bad"] == [] and r["bound_cells"] > 0, r
    if case == "ragged":
        assert r["dims"][2] % 4 != 0, r


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", LEAKING)
def test_device_grid_is_closed_where_the_default_leaks(voxelized, case, prec):
    W.assert_closed(one(voxelized, case, prec)["closed"])


def test_option_zero_is_the_reference_rasteriser(voxelized):
    r = one(voxelized, "sphere-80", "f32")
    assert r["option0_bad"] == [] and r["option0_fluid_cells"] == 0, r      # (the default leaks on this sphere)


# ---- 2. a context updated from the mesh against a fresh upload of the twin's nodes -----------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact", "f32-auto"])
def test_update_from_the_mesh_equals_upload_of_the_conservative_twin(built, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    g1 = nodes_of(W.sphere(80, (30, 38, 30))[0])
    sh, _ = W.sphere(80, (30, 38, 30))
    g = (sh.subframe(0.0)[0] * np.float32(0.9) + np.float32(3.0)).astype(np.float32)       # the same grid, a smaller sphere
    idx = sh.subframe(0.0)[1]
    g2 = nodes_of(W.conservative(sh, g, idx))
    assert not np.array_equal(g1.type, g2.type) and (g2.type == grids.NODE_IN).any()
    lay = M.seeded_layers(g2, dtype)
    a, b = M.make(g1, dtype, kernel, f64_part), M.make(g2, dtype, kernel, f64_part)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    nseg_a = a.update_nodes_shape3d(g, idx, MC.BASE_T, voxels="conservative")
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


# ---- 3. a breathing run ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact"])
def test_breathing_sphere_keeps_its_fluid_and_equals_the_oracle(built, mode):
    """80 faces, r = s (30, 38, 30) about a fixed centre, s from 1.0 to 0.9 and back in 6 steps (the default leaks at 1.0 and
    0.925), G 2 / L 1: NODE_IN stays, the error is finite, the fields equal the CPU oracle driven through the twin's grids."""
    dtype, kernel, f64_part = M.MODES[mode]
    O = M._oracle()
    sh, cell = W.sphere(80, (30, 38, 30))
    g0, idx = sh.subframe(0.0)
    centre = g0.mean(axis=0, dtype=np.float64)
    params = capi.fluid_params(dtype, *M.PARAMS)
    nodes0 = nodes_of(sh)
    a = capi.Solver(nodes0, params, dtype)
    o = O.Oracle(nodes0, params, dtype)
    a.set_option(capi.OPT_SWEEP_KERNEL, kernel); a.set_option(capi.OPT_F64_PART, f64_part); a.set_option(capi.OPT_ERR_ORDER, 1)
    a.set_option(capi.OPT_MESH_VOXELS, 1)
    dt, seen = 0.01, []
    for n, s in enumerate((0.975, 0.95, 0.925, 0.9, 0.95, 1.0)):
        g = ((g0 - centre) * s + centre).astype(np.float32)
        nodes = nodes_of(W.conservative(sh, g, idx))
        seen.append(nodes.type.tobytes())
        a.update_nodes_shape3d(g, idx, MC.BASE_T)
        info = a.geometry_info()
        assert int((nodes.type == grids.NODE_IN).sum()) > 0 and info["bound_cells"] == int((nodes.type == grids.NODE_BOUND).sum())
        a.UpdateBoundaries()
        ea = a.TimeStep(dtype(dt), 2, 1, True)
        assert np.isfinite(ea)
        arrs = [np.ascontiguousarray(nodes.type, np.uint8), np.ascontiguousarray(nodes.bc_vel, np.uint8),
                np.ascontiguousarray(nodes.bc_temp, np.uint8)] + [np.ascontiguousarray(v, dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
        o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in arrs])
        o._f("fs3d_oracle_create_segments")(o.h)
        o.update_boundaries()
        rc, eo = o.time_step(float(dtype(dt)), 2, 1, True)
        assert rc == 0 and eo == ea, (n, eo, ea)
        M.clear_oracle(o, nodes.type == grids.NODE_OUT, MC.BASE_T)
        a.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); a.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        fa = a.download_layer(capi.LAYER_CUR)
        for v, y in enumerate(o.get_layer_fields(O.L_CUR)):
            assert np.array_equal(bits(fa[v]), bits(np.ascontiguousarray(y, dtype))), "step %d field %d differs from the oracle" % (n, v)
    assert len(set(seen)) == 5          # the walls did move (0.95 comes twice)
    a.close(); o.close()


# ---- 4. refusals and the contract ------------------------------------------------------------------------------------------------

def test_option_values_and_the_coordinate_limit(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_EXACT)
    xyz, tri = s._mesh_arrays(g, idx)
    nv, nt = len(xyz[0]), tri.size // 3
    for bad in (2, -1):
        assert s.lib.fs3d_set_option(s.h, capi.OPT_MESH_VOXELS, bad) == capi.ERR_INVALID
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]
    for bad_value in (5000.0, -4097.0, np.nan, np.inf):
        x2 = [a.copy() for a in xyz]; x2[1][7] = bad_value
        st, msg = raw_update(s, x2, nv, tri, nt)
        assert st == capi.ERR_INVALID and "coordinate" in msg and "4096" in msg, (bad_value, st, msg)
    after = s.geometry_info()                    # refused before anything was touched: same tables, nothing counted, the context steps on
    assert [after[k] for k in M.TABLE_KEYS] == [before[k] for k in M.TABLE_KEYS] and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    x2 = [np.append(a, np.float32(v)) for a, v in zip(xyz, (4096.0, -4096.0, 0.0))]      # on the bound (a vertex no triangle uses)
    assert raw_update(s, x2, nv + 1, tri, nt)[0] == capi.OK
    s.set_option(capi.OPT_MESH_VOXELS, 0)        # the default mode keeps its own limit
    x2 = [np.append(a, np.float32(v)) for a, v in zip(xyz, (5000.0, -5000.0, 0.0))]
    assert raw_update(s, x2, nv + 1, tri, nt)[0] == capi.OK
    after = s.geometry_info()
    assert [after[k] for k in M.TABLE_KEYS] == [before[k] for k in M.TABLE_KEYS]
    s.close()


def test_steady_state_allocates_nothing(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = M.make(MC.nodes_of(sh), np.float32, capi.SWEEP_AUTO)
    tw, _ = MC.twin("sphere_3D")
    s.enable_timing(True)
    allocs = []
    for r in range(6):
        s.update_nodes_shape3d(*tw.subframe(0.003 * r), MC.BASE_T, voxels="conservative")
        assert s.last_update_device_ms() > 0
        allocs.append(s.geometry_info()["device_allocs_and_frees"])
    print("allocs + frees after each update:", allocs)
    assert allocs[0] > 0 and all(x == allocs[0] for x in allocs[1:])
    s.close()


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------------

def test_driver_watertight_moving_mesh_equals_host_voxels_and_differs_from_the_default(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    outs = {}
    for word, extra in (("device", ["moving-mesh", "--watertight"]), ("host", ["moving-mesh", "--host-voxels", "--watertight"]), ("default", ["moving-mesh"])):
        prefix = str(tmp_path / word)
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + extra, check=True, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
        errs = re.findall(r"err = ([0-9.]+),", r.stdout)
        n_in = float(re.search(r"NODE_IN points = ([0-9.]+) of total", r.stdout).group(1))
        outs[word] = (errs, n_in, open(prefix + "_res.nc", "rb").read())
    print(outs["device"][:2], outs["default"][:2])
    assert len(outs["device"][0]) in (7, 8) and outs["device"][:2] == outs["host"][:2]
    assert len(outs["device"][2]) > 1000 and outs["device"][2] == outs["host"][2]
    assert 0 < outs["device"][1] < outs["default"][1]                                   # a thicker shell: less fluid
    assert len(outs["default"][2]) == len(outs["device"][2]) and outs["default"][2] != outs["device"][2]


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "voxelize":
        voxelize_all_cases()
