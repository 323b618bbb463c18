"""Moving Shape3D meshes on the GPU: the voxeliser (k_geom_raster_mesh, the flood-fill passes, k_geom_mesh_nodes) against the Python
twin byte for byte and against the reference's own grids, the flood fill alone against scipy's labelling, fs3d_update_nodes_shape3d
against an upload of the twin's nodes bit for bit, a moving run against fs3d_update_nodes and the CPU oracle, the driver's
`moving-mesh` word with and without --host-voxels, and the contract of the three entries (refusals, allocations).
No tolerance appears: everything compared is integers or bit patterns."""
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
from test_gpu_extrude import bare_context  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits


def child(*args):
    """`python tests/test_gpu_mesh.py <what>` in a fresh process in which torch opens the GPU first (see the end of this file)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=900)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


# ---- 1. the voxeliser against the twin -------------------------------------------------------------------------------------------

def voxelize_all_cases():
    """Child process: every case of mesh_cases in fp32 and fp64 through voxelize_shape3d_dev into torch tensors that hold garbage
    before the call; one line per case and precision."""
    import torch
    for case in MC.CASE_IDS:
        sh, g, idx, ref_type = MC.load_case(case)
        want = MC.nodes_of(sh)
        n = want.ncells
        for prec, dtype, td in (("f32", np.float32, torch.float32), ("f64", np.float64, torch.float64)):
            s = bare_context(want.shape, dtype, (sh.dx, sh.dy, sh.dz))
            by = [torch.full((n + 4,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
            va = [torch.full((n + 4,), float("nan"), dtype=td, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            s.voxelize_shape3d_dev(g, idx, MC.BASE_T, *[t[:n] for t in by + va])
            bad = []
            for name, t in zip(MC.NODE_ARRAYS, by + va):
                got = t.cpu().numpy()
                exp = np.ascontiguousarray(getattr(want, name), got.dtype).reshape(-1)
                if not np.array_equal(got[:n].view(np.uint8), exp.view(np.uint8)):
                    bad.append("%s: %d cells" % (name, int((got[:n] != exp).sum())))
                if not (np.isnan(got[n:]).all() if got.dtype.kind == "f" else (got[n:] == 0xAB).all()):
                    bad.append(name + "-outside")
            if ref_type is not None and not np.array_equal(by[0][:n].cpu().numpy(), ref_type.reshape(-1)):
                bad.append("type differs from the reference's grid")
            rec = dict(case=case, prec=prec, dims=list(want.shape), bound_cells=int((want.type == grids.NODE_BOUND).sum()),
                       fluid_cells=int((want.type == grids.NODE_IN).sum()), fill_rounds=s.mesh_fill_rounds(), bad=bad)
            s.close()
            print("CASE " + json.dumps(rec), flush=True)


@pytest.fixture(scope="module")
def voxelized(built):
    return [json.loads(l[5:]) for l in child("voxelize").splitlines() if l.startswith("CASE ")]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", MC.CASE_IDS)
def test_voxeliser_equals_the_twin(voxelized, case, prec):
    mine = [r for r in voxelized if r["case"] == case and r["prec"] == prec]
    assert len(mine) == 1, "the child process did not reach %s %s" % (case, prec)
    assert mine[0]["bad"] == [] and mine[0]["bound_cells"] > 0 and mine[0]["fluid_cells"] > 0, mine[0]


# ---- 2. the flood fill against the labelling -----------------------------------------------------------------------------------

def fill_all_grids():
    import torch
    for name, ty in MC.fill_grids().items():
        s = bare_context(ty.shape, np.float32)
        t = torch.full((ty.size + 4,), 0xAB, dtype=torch.uint8, device="cuda")
        t[:ty.size] = torch.from_numpy(ty.reshape(-1)).cuda()
        torch.cuda.synchronize()
        s.flood_fill_dev(t[:ty.size])
        got = t.cpu().numpy()
        want = MC.label_fill(ty)
        rec = dict(name=name, dims=list(ty.shape), rounds=s.mesh_fill_rounds(), rounds_numpy=MC.pass_fill(ty)[1],
                   differing=int((got[:ty.size] != want.reshape(-1)).sum()), outside_written=bool((got[ty.size:] != 0xAB).any()))
        s.close()
        print("FILL " + json.dumps(rec), flush=True)


@pytest.fixture(scope="module")
def filled(built):
    return {r["name"]: r for r in (json.loads(l[5:]) for l in child("fill").splitlines() if l.startswith("FILL "))}


@pytest.mark.parametrize("name", ["serpentine", "all-in", "bound-at-origin", "two-shells"])
def test_flood_fill_equals_the_labelled_component(filled, name):
    r = filled[name]
    assert r["differing"] == 0 and not r["outside_written"], r
    assert r["rounds"] == r["rounds_numpy"], r          # the same passes in the same order: the same number of rounds
    if name == "serpentine":
        assert r["dims"][2] > 64 and r["dims"][2] % 4 and r["rounds"] > 8, r


# ---- 3. a context updated from the mesh against a fresh upload of the twin's nodes -----------------------------------------------

@pytest.mark.parametrize("mode", list(M.MODES))
def test_update_from_the_mesh_equals_upload(built, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    g1 = MC.nodes_of(MC.load_case("sphere-t0")[0])
    sh, g, idx, _ = MC.load_case("sphere-t2")
    g2 = MC.nodes_of(sh)
    assert not np.array_equal(g1.type, g2.type)
    lay = M.seeded_layers(g2, dtype)
    a, b = M.make(g1, dtype, kernel, f64_part), M.make(g2, dtype, kernel, f64_part)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    nseg_a = a.update_nodes_shape3d(g, idx, MC.BASE_T)
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


# ---- 4. a moving run -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact", "f32-auto"])
def test_moving_run_equals_update_from_the_nodes_and_the_oracle(built, mode):
    """The sphere through 6 steps of its own run (dt = frame_time / (frames * time_steps); the sub-frame passes from frame 1 to
    frame 0 on the way): one context takes the mesh per step, the other the twin's nodes, the CPU oracle the same nodes."""
    dtype, kernel, f64_part = M.MODES[mode]
    O = M._oracle()
    sh, fx = MC.twin("sphere_3D")
    cfg = fx.cfg()
    dt = cfg.frame_time / (len(sh.frames) * cfg.time_steps)
    params = capi.fluid_params(dtype, cfg.Re, cfg.Pr, cfg.lam)
    nodes0 = MC.nodes_of(sh)
    a, b = capi.Solver(nodes0, params, dtype), capi.Solver(nodes0, params, dtype)
    exact = kernel == capi.SWEEP_EXACT
    o = O.Oracle(nodes0, params, dtype) if exact else None
    for s in (a, b):
        s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
        s.set_option(capi.OPT_F64_PART, f64_part)
        if exact:
            s.set_option(capi.OPT_ERR_ORDER, 1)      # the reported error in the CPU path's summation order: bit-equal too
    seen = []
    for n in range(6):
        t = dt * (n + 1)
        g, idx = sh.subframe(t)
        sh.build(g, idx)
        nodes = MC.nodes_of(sh)
        seen.append(nodes.type.copy())
        nseg_a, nseg_b = a.update_nodes_shape3d(g, idx, MC.BASE_T), b.update_nodes(nodes)
        assert nseg_a == nseg_b
        a.UpdateBoundaries(); b.UpdateBoundaries()
        ea, eb = a.TimeStep(dtype(dt), cfg.num_global, cfg.num_local, True), b.TimeStep(dtype(dt), cfg.num_global, cfg.num_local, True)
        assert ea == eb, (n, ea, eb)
        if exact:
            arrs = [np.ascontiguousarray(nodes.type, np.uint8), np.ascontiguousarray(nodes.bc_vel, np.uint8),
                    np.ascontiguousarray(nodes.bc_temp, np.uint8)] + [np.ascontiguousarray(v, dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
            o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in arrs])
            o._f("fs3d_oracle_create_segments")(o.h)
            o.update_boundaries()
            rc, eo = o.time_step(float(dtype(dt)), cfg.num_global, cfg.num_local, True)
            assert rc == 0 and eo == ea, (n, eo, ea)
            M.clear_oracle(o, nodes.type == grids.NODE_OUT, cfg.baseT)
        for s in (a, b):
            s.clear_outer_cells(capi.LAYER_NEXT, cfg.baseT); s.clear_outer_cells(capi.LAYER_CUR, cfg.baseT)
        fa, fb = a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR)
        for v in range(4):
            assert np.array_equal(bits(fa[v]), bits(fb[v])), "step %d field %d: %d cells differ" % (n, v, int((bits(fa[v]) != bits(fb[v])).sum()))
        if exact:
            for v, y in enumerate(o.get_layer_fields(O.L_CUR)):
                assert np.array_equal(bits(fa[v]), bits(np.ascontiguousarray(y, dtype))), "step %d field %d differs from the oracle" % (n, v)
    assert len({x.tobytes() for x in seen}) >= 4          # the walls did move
    a.close(); b.close()
    if o:
        o.close()


# ---- 5. the driver -------------------------------------------------------------------------------------------------------------

def test_driver_moving_mesh_equals_host_voxels_and_differs_from_the_static_run(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    outs = {}
    for word, extra in (("device", ["moving-mesh"]), ("host", ["moving-mesh", "--host-voxels"]), ("static", [])):
        prefix = str(tmp_path / word)
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + extra, check=True, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
        errs = re.findall(r"err = ([0-9.]+),", r.stdout)
        n_cs = int(re.search(r"CreateSegments\s+[0-9.]+\s+[0-9.]+\s+(\d+)", r.stdout).group(1))
        outs[word] = (errs, n_cs, open(prefix + "_res.nc", "rb").read())
    print(outs["device"][:2], outs["static"][:2])
    n = len(outs["device"][0])
    assert n in (7, 8) and outs["device"][1] == n + 1 and outs["static"][1] == 1
    assert outs["device"][:2] == outs["host"][:2]
    assert len(outs["device"][2]) > 1000 and outs["device"][2] == outs["host"][2]
    assert len(outs["static"][2]) == len(outs["device"][2]) and outs["static"][2] != outs["device"][2]      # the walls do move


# ---- 6. refusals and the contract ------------------------------------------------------------------------------------------------

def sphere_context(kernel=capi.SWEEP_EXACT):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    return M.make(MC.nodes_of(sh), np.float32, kernel), g, idx


def raw_update(s, xyz, nvert, tri, ntri):
    nseg = (C.c_int * 3)()
    st = s.lib.fs3d_update_nodes_shape3d(s.h, *[capi._p(a) for a in xyz], nvert, capi._p(tri), ntri, 1.0, nseg)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


def test_invalid_meshes_are_refused_and_the_context_keeps_its_geometry(built):
    s, g, idx = sphere_context()
    xyz, tri = s._mesh_arrays(g, idx)
    nv, nt = len(xyz[0]), tri.size // 3
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]
    for hole in range(4):                                          # NULL, each array in turn
        arrs = [None if q == hole else a for q, a in enumerate(xyz + [tri])]
        st, msg = raw_update(s, arrs[:3], nv, arrs[3], nt)
        assert st == capi.ERR_INVALID and "NULL" in msg, (hole, st, msg)
        assert s.lib.fs3d_voxelize_shape3d_dev(s.h, *[capi._p(a) for a in arrs[:3]], nv, capi._p(arrs[3]), nt, 1.0, *[None] * 7) == capi.ERR_INVALID
    assert s.lib.fs3d_voxelize_shape3d_dev(s.h, *[capi._p(a) for a in xyz], nv, capi._p(tri), nt, 1.0, *[None] * 7) == capi.ERR_INVALID
    assert b"NULL" in s.lib.fs3d_last_error(s.h)
    assert s.lib.fs3d_flood_fill_dev(s.h, None) == capi.ERR_INVALID and b"NULL" in s.lib.fs3d_last_error(s.h)
    assert raw_update(s, xyz, 0, tri, nt)[0] == capi.ERR_INVALID
    assert raw_update(s, xyz, nv, tri, -1)[0] == capi.ERR_INVALID
    for bad_index in (-1, nv):
        t2 = tri.copy(); t2[5] = bad_index
        st, msg = raw_update(s, xyz, nv, t2, nt)
        assert st == capi.ERR_INVALID and "index" in msg, (st, msg)
    for bad_value in (np.nan, np.inf, -np.inf, 65537.0, -70000.0):
        for axis in range(3):
            x2 = [a.copy() for a in xyz]; x2[axis][7] = bad_value
            st, msg = raw_update(s, x2, nv, tri, nt)
            assert st == capi.ERR_INVALID and "coordinate" in msg, (bad_value, axis, st, msg)
    # refused before anything was touched: same tables, nothing counted, and the context still steps
    after = s.geometry_info()
    assert [after[k] for k in M.TABLE_KEYS] == [before[k] for k in M.TABLE_KEYS] and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    # a coordinate on the bound is taken (a vertex no triangle uses), and so is a mesh without triangles: nothing but NODE_OUT
    x2 = [np.append(a, np.float32(v)) for a, v in zip(xyz, (65536.0, -65536.0, 0.0))]
    assert raw_update(s, x2, nv + 1, tri, nt)[0] == capi.OK
    after = s.geometry_info()
    assert [after[k] for k in M.TABLE_KEYS] == [before[k] for k in M.TABLE_KEYS]
    assert raw_update(s, xyz, nv, tri, 0)[0] == capi.OK and s.geometry_info()["bound_cells"] == 0
    s.close()


def test_scan_line_guard_refuses_the_mesh_and_leaves_no_geometry(built):
    """shape3d.py raises on this mesh (tests/test_mesh_api.py); the kernel stops the triangle and the host turns its flag into
    FS3D_ERR_INVALID with the twin's message.  Finite and inside the coordinate bound, so the check is not skipped."""
    s, g, idx = sphere_context()
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes_shape3d(*MC.long_scan_line_mesh(), MC.BASE_T)
    assert ei.value.status == capi.ERR_INVALID and "never reaches its end cell" in str(ei.value)
    for call in (lambda: s.TimeStep(np.float32(M.DT), 1, 1, True), s.UpdateBoundaries, s.geometry_info):
        with pytest.raises(capi.Fs3dError) as ei:
            call()
        assert ei.value.status == capi.ERR_INVALID and "upload nodes" in str(ei.value)
    s.update_nodes_shape3d(g, idx, MC.BASE_T)                     # an update that succeeds brings the geometry back
    fresh = sphere_context()[0]
    ia, ib = s.geometry_info(), fresh.geometry_info()
    assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    s.close(); fresh.close()


def test_update_before_any_upload_is_invalid(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = bare_context(sh.type.shape, np.float32)
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes_shape3d(g, idx, MC.BASE_T)
    assert ei.value.status == capi.ERR_INVALID and "fs3d_upload_nodes" in str(ei.value)
    s.close()


def test_mesh_entries_on_a_slab_context_are_unsupported(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    s = capi.Solver(MC.nodes_of(sh), capi.fluid_params(np.float32, *M.PARAMS), np.float32, x_range=(0, 16))
    xyz, tri = s._mesh_arrays(g, idx)
    st, msg = raw_update(s, xyz, len(xyz[0]), tri, tri.size // 3)
    assert st == capi.ERR_UNSUPPORTED and "single context" in msg
    one = np.zeros(8, np.uint8)                                    # never read: refused before anything is launched
    assert s.lib.fs3d_voxelize_shape3d_dev(s.h, *[capi._p(a) for a in xyz], len(xyz[0]), capi._p(tri), tri.size // 3, 1.0, *[capi._p(one)] * 7) == capi.ERR_UNSUPPORTED
    assert b"single context" in s.lib.fs3d_last_error(s.h)
    assert s.lib.fs3d_flood_fill_dev(s.h, capi._p(one)) == capi.ERR_UNSUPPORTED and b"single context" in s.lib.fs3d_last_error(s.h)
    s.UpdateBoundaries()                 # refused before anything was touched: the slab keeps its geometry
    s.close()


def test_steady_state_allocates_nothing_and_updates_are_counted(built):
    s, _, _ = sphere_context(capi.SWEEP_AUTO)
    sh, _ = MC.twin("sphere_3D")
    s.enable_timing(True)
    allocs = []
    for r in range(11):
        s.update_nodes_shape3d(*sh.subframe(0.003 * r), MC.BASE_T)
        assert s.last_update_device_ms() > 0
        allocs.append(s.geometry_info()["device_allocs_and_frees"])
    print("allocs + frees after each update:", allocs)
    assert allocs[0] > 0 and all(x == allocs[0] for x in allocs[1:])
    assert s.profiler_events()["CreateSegments"][1] == 12
    s.close()


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "voxelize":
        voxelize_all_cases()
    elif sys.argv[1] == "fill":
        fill_all_grids()
