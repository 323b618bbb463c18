"""Moving Shape3D meshes on x-slabs (include/fs3d.h): fs3d_update_nodes_shape3d_slab / fs3d_update_nodes_shape3d_vel_slab
voxelise and flood-fill the GLOBAL grid on every rank's own device, without talking to any other rank, and build the tables
fs3d_upload_nodes builds for the slab's planes from the twin's global nodes.  Everything is held bit for bit: the tables to a fresh
slab context that uploaded the twin's nodes, the time steps of a group to a single context that took the same meshes through
fs3d_update_nodes_shape3d_vel.  No tolerance is introduced; the reported error of a group is compared as
tests/test_gpu_slab_geometry.py compares it (rtol 1e-12: the slabs add their partial sums in another order than one context adds
its own, and only that).  Cases: tests/mesh_slab_cases.py; their conditions are asserted in tests/test_mesh_slab_api.py."""
import ctypes as C
import functools
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
import slab_geometry_cases as SC  # noqa: E402
import test_gpu_moving as M  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
from test_gpu_slab_geometry import assert_same_context, bits, params, tables  # noqa: E402
from cmc_fluid_solver_amd import capi, grids  # noqa: E402

pytestmark = pytest.mark.gpu

DT = 0.1
LAYERS = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF, capi.LAYER_NEXT)
PLAIN, VEL = "fs3d_update_nodes_shape3d_slab", "fs3d_update_nodes_shape3d_vel_slab"


@pytest.fixture(autouse=True)
def _exact_kernels(monkeypatch):
    """New contexts start on the bit-exact kernels (FS3D_SWEEP_EXACT); the test of the default kernels selects them itself."""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")


def bare_slab_context(gdims, xr, dtype=np.float32):
    """A context for the planes xr of a grid of gdims, without geometry."""
    s = capi.Solver.__new__(capi.Solver)
    s.lib, s.dtype = capi.load(), np.dtype(dtype)
    s.prec = capi.F32 if s.dtype == np.float32 else capi.F64
    s.gdims = tuple(gdims)
    s.dims = (xr[1] - xr[0],) + tuple(gdims[1:])
    s.x0, s.x1 = xr
    s.h = C.c_void_p()
    st = s.lib.fs3d_create(C.byref(s.h), 0, s.prec, xr[1] - xr[0], gdims[1], gdims[2], 0.1, 0.1, 0.1, xr[0], gdims[0])
    assert st == capi.OK, s.lib.fs3d_last_error(None)
    return s


# ---- 1. the tables of a slab context updated from the mesh equal those of a fresh upload of the twin's nodes ------------------
# (2. the fill is global: the case tube-cube, whose middle slab a slab-local fill would leave full of NODE_IN cells)

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,nranks", [(n, r) for n in MS.TABLE_CASES for r in MS.RANKS[n]])
def test_slab_update_from_the_mesh_equals_a_fresh_upload(built, name, nranks, dtype):
    case = MS.case(name)
    start = case.start()
    for xr in MS.ranges(case.want.dimx, nranks):
        s = capi.Solver(start, params(dtype), dtype, x_range=xr)
        nseg = case.update(s)
        f = capi.Solver(case.want, params(dtype), dtype, x_range=xr)
        print(name, nranks, xr, case.want.shape, tables(s), "fill rounds", s.mesh_fill_rounds())
        assert nseg == f.num_segments
        assert_same_context(s, f, "%s, planes %s of %d ranks" % (name, xr, nranks))
        s.close(); f.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nranks", MS.RANKS["sphere-80-zero"])
def test_zero_velocities_and_wall_temperature_zero_equal_the_plain_slab_entry(built, nranks, dtype):
    case = MS.case("sphere-80-zero")
    start = case.start()
    for xr in MS.ranges(case.want.dimx, nranks):
        a, b = (capi.Solver(start, params(dtype), dtype, x_range=xr) for _ in range(2))
        nseg = case.update(a)
        assert nseg == b.update_nodes_shape3d_slab(case.g, case.idx, MC.BASE_T, voxels=case.voxels)
        assert_same_context(a, b, "planes %s of %d ranks" % (xr, nranks))
        a.close(); b.close()


def child(*args):
    """`python tests/test_gpu_mesh_slab.py <what>` in a fresh process in which torch opens the GPU first (see the end of this file)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def fill_from_a_slab():
    import torch
    ty = MC.serpentine()
    assert ty.shape[0] == 24
    s = bare_slab_context(ty.shape, (8, 16))
    t = torch.full((ty.size + 4,), 0xAB, dtype=torch.uint8, device="cuda")
    t[:ty.size] = torch.from_numpy(ty.reshape(-1)).cuda()
    torch.cuda.synchronize()
    s.flood_fill_global_dev(t[:ty.size])
    got = t.cpu().numpy()
    want = MC.label_fill(ty)
    rec = dict(dims=list(ty.shape), rounds=s.mesh_fill_rounds(), rounds_numpy=MC.pass_fill(ty)[1],
               differing=int((got[:ty.size] != want.reshape(-1)).sum()), outside_written=bool((got[ty.size:] != 0xAB).any()),
               turned_outside_the_slab=int((want[:8] != ty[:8]).sum() + (want[16:] != ty[16:]).sum()))
    s.close()
    print("FILL " + json.dumps(rec), flush=True)


def test_flood_fill_from_a_slab_context_covers_the_global_grid(built):
    r = [json.loads(l[5:]) for l in child("fill").splitlines() if l.startswith("FILL ")]
    assert len(r) == 1, "the child process did not reach the fill"
    r = r[0]
    assert r["differing"] == 0 and not r["outside_written"], r
    assert r["rounds"] == r["rounds_numpy"] and r["turned_outside_the_slab"] > 0, r


# ---- 3. time steps of a group, bit for bit -----------------------------------------------------------------------------------------

def run_translating(s, dtype, update):
    """every geometry of the translating sphere: the update, a time step, ClearOutterCells on next and cur; cur after every step"""
    curs, errs = [], []
    for nodes, g, vel, idx in WV.translating_grids():
        update(g, vel, idx, MC.BASE_T, MC.BASE_T, voxels="conservative")
        s.UpdateBoundaries()
        errs.append(s.TimeStep(dtype(WV.RUN_DT), WV.RUN_GL[0], WV.RUN_GL[1], True))
        s.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); s.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        curs.append(s.download_layer(capi.LAYER_CUR))
    return curs, errs


@functools.lru_cache(maxsize=None)
def translating_single(dtype):
    s = capi.Solver(WV.translating_grids()[0][0], params(dtype), dtype)
    out = run_translating(s, dtype, s.update_nodes_shape3d_vel)
    s.close()
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_group_steps_through_the_translating_sphere_equal_the_single_context(built, nranks, dtype):
    ref, ref_err = translating_single(dtype)
    grp = capi.LocalGroup(WV.translating_grids()[0][0], params(dtype), nranks, dtype)
    res = grp.run(lambda rank, s: run_translating(s, dtype, s.update_nodes_shape3d_vel_slab))
    grp.close()
    for n in range(WV.RUN_STEPS):
        for v in range(4):
            got = np.concatenate([res[r][0][n][v] for r in range(nranks)], axis=0)
            assert np.array_equal(bits(ref[n][v]), bits(got)), "step %d field %d differs in %d cells" % (n, v, int((bits(ref[n][v]) != bits(got)).sum()))
    for r in range(nranks):                                   # every rank holds the global error
        print(nranks, r, res[r][1], ref_err)
        np.testing.assert_allclose(res[r][1], ref_err, rtol=1e-12)


def test_default_kernels_after_a_mesh_update_equal_a_fresh_group(built, monkeypatch):
    """sphere-t0 -> sphere-t2 through the plain entry, on FS3D_SWEEP_AUTO: the pattern of
    test_gpu_slab_geometry.py::test_default_kernels_after_an_update_equal_a_fresh_group."""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", str(capi.SWEEP_AUTO))
    dtype, nranks = np.float32, 3
    A = MC.nodes_of(MC.load_case("sphere-t0")[0])
    sh, g, idx, _ = MC.load_case("sphere-t2")
    B = MC.nodes_of(sh)

    def two_steps(s):
        errs = []
        for _ in range(2):
            s.UpdateBoundaries(); errs.append(s.TimeStep(dtype(DT), 2, 2, True))
        return s.download_layer(capi.LAYER_CUR), errs, s.last_sweep_kernels()

    def updated(rank, s):
        for _ in range(2):
            s.UpdateBoundaries(); s.TimeStep(dtype(DT), 2, 2, True)
        s.update_nodes_shape3d_slab(g, idx, MC.BASE_T, voxels="reference")
        s.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T); s.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T)
        return {l: s.download_layer(l) for l in LAYERS}, two_steps(s)

    ga = capi.LocalGroup(A, params(dtype), nranks, dtype)
    got = ga.run(updated)
    ga.close()

    def fresh(rank, s):
        for l in LAYERS:
            s.upload_layer(l, got[rank][0][l])
        return two_steps(s)
    gb = capi.LocalGroup(B, params(dtype), nranks, dtype)
    want = gb.run(fresh)
    gb.close()
    for r in range(nranks):
        (cur_a, err_a, ran_a), (cur_b, err_b, ran_b) = got[r][1], want[r]
        print(r, ran_a, err_a, err_b)
        assert ran_a == ran_b and "part" in "".join(ran_a.values()), (ran_a, ran_b)
        assert err_a == err_b
        for v in range(4):
            assert np.array_equal(bits(cur_a[v]), bits(cur_b[v])), "rank %d field %d differs in %d cells" % (r, v, int((bits(cur_a[v]) != bits(cur_b[v])).sum()))


# ---- 4. a whole-grid context ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("entry", ["plain", "vel"])
def test_whole_grid_context_takes_the_slab_entries(built, entry, dtype):
    if entry == "plain":
        g1 = MC.nodes_of(MC.load_case("sphere-t0")[0])
        sh, g, idx, _ = MC.load_case("sphere-t2")
        g2 = MC.nodes_of(sh)
        calls = (lambda s: s.update_nodes_shape3d_slab(g, idx, MC.BASE_T, voxels="reference"),
                 lambda s: s.update_nodes_shape3d(g, idx, MC.BASE_T, voxels="reference"))
    else:
        steps = WV.translating_grids()
        g1, (g2, g, vel, idx) = steps[0][0], steps[5]
        calls = (lambda s: s.update_nodes_shape3d_vel_slab(g, vel, idx, MC.BASE_T, WV.WALL_T, voxels="conservative"),
                 lambda s: s.update_nodes_shape3d_vel(g, vel, idx, MC.BASE_T, WV.WALL_T, voxels="conservative"))
    lay = M.seeded_layers(g2, dtype)
    a, b = M.make(g1, dtype, capi.SWEEP_EXACT), M.make(g1, dtype, capi.SWEEP_EXACT)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    assert calls[0](a) == calls[1](b)
    assert tables(a) == tables(b) and tables(a)["segments_z"] > 0
    for step in range(3):
        a.UpdateBoundaries(); b.UpdateBoundaries()
        a.TimeStep(dtype(DT), 2, 2, False); b.TimeStep(dtype(DT), 2, 2, False)
    for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
        assert np.array_equal(bits(x), bits(y)), "field %d differs in %d cells" % (v, int((bits(x) != bits(y)).sum()))
    assert_same_context(a, b, entry)
    a.close(); b.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------

def raw_plain(s, xyz, nvert, tri, ntri):
    nseg = (C.c_int * 3)()
    st = s.lib.fs3d_update_nodes_shape3d_slab(s.h, *[capi._p(a) for a in xyz], nvert, capi._p(tri), ntri, 1.0, nseg)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


def raw_vel(s, xyz, w, nvert, tri, ntri, wallT=WV.WALL_T):
    nseg = (C.c_int * 3)()
    st = s.lib.fs3d_update_nodes_shape3d_vel_slab(s.h, *[capi._p(a) for a in list(xyz) + list(w)], nvert, capi._p(tri), ntri, 1.0, wallT, nseg)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


def refusals_on(rank, s):
    """every refusal that comes before the geometry is given up, on one member of a group; then the group steps"""
    g, idx = MS.tube_cube_mesh()
    g = (g * np.float32(0.4)).astype(np.float32)               # inside the 12^3 grid
    xyz, tri = s._mesh_arrays(g, idx)
    w = s._mesh_velocities(WV.velocities(g) * np.float32(2.0 ** -10), len(xyz[0]))
    nv, nt = len(xyz[0]), tri.size // 3
    before, n_before = tables(s), s.profiler_events()["CreateSegments"][1]
    seen = []

    def refused(res, entry, word):
        st, msg = res
        seen.append((st, msg))
        assert st == capi.ERR_INVALID and msg.startswith(entry + ":") and word in msg, (st, msg)
        assert tables(s) == before and s.profiler_events()["CreateSegments"][1] == n_before, msg

    refused(raw_vel(s, xyz, w, nv, tri, nt), VEL, "conservative")                                       # FS3D_OPT_MESH_VOXELS is 0
    for hole in range(4):                                                                               # NULL, each array in turn
        arrs = [None if q == hole else a for q, a in enumerate(xyz + [tri])]
        refused(raw_plain(s, arrs[:3], nv, arrs[3], nt), PLAIN, "NULL array")
    for bad_index in (-1, nv):
        t2 = tri.copy(); t2[5] = bad_index
        refused(raw_plain(s, xyz, nv, t2, nt), PLAIN, "index")
    for bad_value in (np.nan, np.inf, -np.inf, 65537.0):
        x2 = [a.copy() for a in xyz]; x2[1][7] = bad_value
        refused(raw_plain(s, x2, nv, tri, nt), PLAIN, "coordinate")
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    for entry, call in ((PLAIN, lambda x: raw_plain(s, x, nv, tri, nt)), (VEL, lambda x: raw_vel(s, x, w, nv, tri, nt))):
        x2 = [a.copy() for a in xyz]; x2[0][3] = 4097.0                                                 # finite, inside the rasteriser's bound
        refused(call(x2), entry, "4096")
    for hole in range(3):                                                                               # NULL, each velocity array in turn
        refused(raw_vel(s, xyz, [None if q == hole else a for q, a in enumerate(w)], nv, tri, nt), VEL, "NULL array")
    for bad_value in (np.nan, np.inf, -np.inf):
        w2 = [a.copy() for a in w]; w2[2][5] = bad_value
        refused(raw_vel(s, xyz, w2, nv, tri, nt), VEL, "velocity")
    for bad_value in (np.nan, np.inf):
        refused(raw_vel(s, xyz, w, nv, tri, nt, wallT=bad_value), VEL, "temperature")
    s.UpdateBoundaries()
    err = s.TimeStep(np.float32(DT), 1, 1, True)              # the slab still steps, with its group
    st, msg = raw_vel(s, xyz, w, nv, tri, nt)                  # and the same call with nothing wrong goes through
    assert st == capi.OK, msg
    assert s.profiler_events()["CreateSegments"][1] == n_before + 1
    return (s.x0, s.x1), len(seen), err


def test_refusals_leave_the_slab_as_it_was(built):
    grp = capi.LocalGroup(grids.box(*SC.REFUSAL_DIMS), params(np.float32), 3, np.float32)
    res = grp.run(refusals_on)
    grp.close()
    print(res)
    assert [r[0] for r in res] == [(0, 4), (4, 8), (8, 12)] and all(r[1] == 21 and np.isfinite(r[2]) for r in res)


def test_no_mesh_update_on_a_slab_before_the_first_upload(built):
    g, idx = MS.tube_cube_mesh()
    s = bare_slab_context(MS.TUBE_DIMS, MS.TUBE_SLAB)
    xyz, tri = s._mesh_arrays(g, idx)
    w = s._mesh_velocities(np.zeros_like(g), len(xyz[0]))
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    for (st, msg), entry in ((raw_plain(s, xyz, len(xyz[0]), tri, tri.size // 3), PLAIN), (raw_vel(s, xyz, w, len(xyz[0]), tri, tri.size // 3), VEL)):
        assert st == capi.ERR_INVALID and msg.startswith(entry + ":") and "upload nodes first" in msg, (st, msg)
    assert s.profiler_events()["CreateSegments"][1] == 0
    s.close()


def test_scan_line_guard_names_the_slab_entry_and_leaves_no_geometry(built):
    sh, g, idx, _ = MC.load_case("sphere-t0")
    nodes, xr = MC.nodes_of(sh), (8, 24)
    s = capi.Solver(nodes, params(np.float32), np.float32, x_range=xr)
    n_before = s.profiler_events()["CreateSegments"][1]
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes_shape3d_slab(*MC.long_scan_line_mesh(), MC.BASE_T, voxels="reference")
    print(ei.value)
    assert ei.value.status == capi.ERR_INVALID and (PLAIN + ":") in str(ei.value) and "never reaches its end cell" in str(ei.value)
    for call in (s.UpdateBoundaries, s.geometry_info):
        with pytest.raises(capi.Fs3dError) as ei:
            call()
        assert ei.value.status == capi.ERR_INVALID and "upload nodes" in str(ei.value)
    assert s.profiler_events()["CreateSegments"][1] == n_before
    s.update_nodes_shape3d_slab(g, idx, MC.BASE_T)              # an update that succeeds brings the geometry back
    fresh = capi.Solver(nodes, params(np.float32), np.float32, x_range=xr)
    assert_same_context(s, fresh, "restored")
    assert s.profiler_events()["CreateSegments"][1] == n_before + 1
    # the entries without _slab still refuse a slab
    xyz, tri = s._mesh_arrays(g, idx)
    w = s._mesh_velocities(np.zeros_like(g), len(xyz[0]))
    nseg = (C.c_int * 3)()
    assert s.lib.fs3d_update_nodes_shape3d(s.h, *[capi._p(a) for a in xyz], len(xyz[0]), capi._p(tri), tri.size // 3, 1.0, nseg) == capi.ERR_UNSUPPORTED
    assert b"single context" in s.lib.fs3d_last_error(s.h)
    assert s.lib.fs3d_update_nodes_shape3d_vel(s.h, *[capi._p(a) for a in xyz + w], len(xyz[0]), capi._p(tri), tri.size // 3, 1.0, 0.0, nseg) == capi.ERR_UNSUPPORTED
    assert b"single context" in s.lib.fs3d_last_error(s.h)
    assert_same_context(s, fresh, "after the old entries' refusals")
    s.close(); fresh.close()


# ---- 6. steady state ------------------------------------------------------------------------------------------------------------------------

def test_no_allocation_after_the_second_mesh_update_of_a_slab(built):
    steps = WV.translating_grids()
    xr = MS.ranges(steps[0][0].dimx, 2)[1]
    p, v = (capi.Solver(steps[0][0], params(np.float32), np.float32, x_range=xr) for _ in range(2))
    for s in (p, v):
        s.enable_timing(True)
    n_before = v.profiler_events()["CreateSegments"][1]
    counts_p, counts_v = [], []
    for k in range(4):
        nodes, g, vel, idx = steps[2 * k]
        p.update_nodes_shape3d_slab(g, idx, MC.BASE_T, voxels="conservative")
        v.update_nodes_shape3d_vel_slab(g, vel, idx, MC.BASE_T, MC.BASE_T, voxels="conservative")
        assert p.last_update_device_ms() > 0 and v.last_update_device_ms() > 0
        counts_p.append(p.geometry_info()["device_allocs_and_frees"]); counts_v.append(v.geometry_info()["device_allocs_and_frees"])
    print(counts_p, counts_v)
    assert counts_p[1] == counts_p[3] and counts_v[1] == counts_v[3]
    assert counts_v[0] == counts_p[0] + 1                       # the owner array, 4 bytes per cell of the slab, comes with the first _vel call
    assert v.profiler_events()["CreateSegments"][1] == n_before + 4
    p.close(); v.close()


# ---- 7. the driver ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    from cmc_fluid_solver_amd import build as B
    return B.build_driver()


WORDS = ["moving-mesh", "--watertight", "--wall-velocity", "motion", "--steps", "6"]


@pytest.fixture(scope="module")
def sphere_single(driver, tmp_path_factory):
    import test_host_driver_moving_slabs as D
    return D.run(driver, tmp_path_factory.mktemp("sphere"), "one", D.SPHERE, ["GPU"] + WORDS)


@pytest.mark.parametrize("n", ["2", "3"])
def test_driver_slab_voxels_equals_the_single_gpu_run(driver, sphere_single, n, tmp_path):
    import test_host_driver_moving_slabs as D
    words = ["GPU", n, "--same-device", "moving-mesh", "--slab-voxels"] + WORDS[1:]
    D.assert_same_run(sphere_single, D.run(driver, tmp_path, "slabs", D.SPHERE, words), 6)


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "fill":
        fill_from_a_slab()
