"""The extrusion of a Shape2D grid on the device (k_geom_extrude): fs3d_extrude_shape2d_dev against the numpy rule byte for byte,
fs3d_update_nodes_shape2d against fs3d_update_nodes with the host-extruded nodes bit for bit, the driver's `moving` word with
and without --host-extrusion, and the contract of fs3d_update_nodes* (allocations, refusals, the CreateSegments count).
No tolerance appears: the feature moves bytes and has no arithmetic of its own."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:          # run as a script (the child process below)
    sys.path.insert(0, os.path.dirname(HERE))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import extrude_cases as EC  # noqa: E402
import test_gpu_moving as M  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape2d  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits


def child(*args):
    """`python tests/test_gpu_extrude.py <what> ...` in a fresh process in which torch opens the GPU first (see the end of this file)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=900)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def bare_context(dims, dtype, spacing=(0.1, 0.1, 0.1)):
    """A context without geometry (fs3d_extrude_shape2d_dev needs none; the degenerate grids have no fluid to upload)."""
    s = capi.Solver.__new__(capi.Solver)
    s.lib, s.dtype = capi.load(), np.dtype(dtype)
    s.prec = capi.F32 if s.dtype == np.float32 else capi.F64
    s.dims = s.gdims = tuple(dims)
    s.x0, s.x1 = 0, dims[0]
    s.h = C.c_void_p()
    st = s.lib.fs3d_create(C.byref(s.h), 0, s.prec, dims[0], dims[1], dims[2], *spacing, 0, dims[0])
    assert st == capi.OK, s.lib.fs3d_last_error(None)
    return s


# ---- 1. the kernel against the rule ------------------------------------------------------------------------------------------

def extrude_all_cases(prec):
    """Child process (torch opens the GPU first): every case of extrude_cases through extrude_shape2d_dev into torch tensors that
    hold garbage before the call; one line per case."""
    import torch
    dtype = np.float32 if prec == "f32" else np.float64
    td = torch.float32 if prec == "f32" else torch.float64
    for case in EC.CASE_IDS:
        nodes, g2, p = EC.load_case(case)
        want = EC.twin(g2, p)
        if want.dimz < 3:          # fs3d_create takes no grid of fewer than 3 cells in z: active_dimz 2 without `align` runs in dimz 3 (one more lid cell)
            want = shape2d.extrude_grid2d(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"], dimz=3)
        n = want.ncells
        # (bytes, values) the arrays start after their buffers do: (1, 1) off every alignment (one cell per thread); (4, 2) the least
        # alignment of the 4-cells-per-thread path -- byte arrays on 4 bytes, fp64 arrays on 16 but not 32 (fp32 ones on 8: one cell per thread)
        for shifts in (((0, 0), (1, 1), (4, 2)) if case in ("heart_us-t3", "adz5-var3-align") else ((0, 0),)):
            s = bare_context(want.shape, dtype, (p["dx"], p["dy"], p["dz"]))
            by = [torch.full((n + 4,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
            va = [torch.full((n + 4,), float("nan"), dtype=td, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            sh = [shifts[0]] * 3 + [shifts[1]] * 4
            if any(sh):
                outs = [t.data_ptr() + q * t.element_size() for t, q in zip(by + va, sh)]
            else:
                outs = [t[:n] for t in by + va]
            s.extrude_shape2d_dev(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"], *outs)
            bad = []
            for name, t, shift in zip(EC.NODE_ARRAYS, by + va, sh):
                got = t.cpu().numpy()
                exp = np.ascontiguousarray(getattr(want, name), got.dtype).reshape(-1)
                if not np.array_equal(got[shift:shift + n].view(np.uint8), exp.view(np.uint8)):
                    bad.append(name)
                # nothing outside the n cells is written
                pad = np.concatenate([got[:shift], got[shift + n:]])
                if not (np.isnan(pad).all() if pad.dtype.kind == "f" else (pad == 0xAB).all()):
                    bad.append(name + "-outside")
            s.close()
            print("CASE " + json.dumps(dict(case=case, shift=list(shifts), dims=list(want.shape), bad=bad)), flush=True)


@pytest.fixture(scope="module")
def extruded_f32(built):
    return [json.loads(l[5:]) for l in child("extrude", "f32").splitlines() if l.startswith("CASE ")]


@pytest.fixture(scope="module")
def extruded_f64(built):
    return [json.loads(l[5:]) for l in child("extrude", "f64").splitlines() if l.startswith("CASE ")]


def _case_ok(rec, case):
    mine = [r for r in rec if r["case"] == case]
    assert mine, "the child process did not reach %s" % case
    for r in mine:
        assert r["bad"] == [], r


@pytest.mark.parametrize("case", EC.CASE_IDS)
def test_extrusion_equals_the_rule_f32(extruded_f32, case): _case_ok(extruded_f32, case)


@pytest.mark.parametrize("case", EC.CASE_IDS)
def test_extrusion_equals_the_rule_f64(extruded_f64, case): _case_ok(extruded_f64, case)


# ---- 2. a context updated from the 2D grid against one updated from the host-extruded nodes -------------------------------------

def geometry(name):
    """(nodes the contexts start from, nodes at the case's time, Grid2D at that time, params)"""
    if name == "non_uniform_pipe":
        nodes, g2, p = EC.load_case(name)
        start = grids.box(*nodes.shape, h=p["dx"])                 # same dims and spacing, another geometry
        start.dx, start.dy, start.dz = nodes.dx, nodes.dy, nodes.dz
        return start, nodes, g2, p
    nodes, g2, p = EC.load_case(name)
    return EC.load_case("heart_us-t0")[0], nodes, g2, p


@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact", "f32-auto"])
@pytest.mark.parametrize("name", ["heart_us-t3", "heart_us-t5", "non_uniform_pipe"])
def test_update_from_the_2d_grid_equals_update_from_the_nodes(built, name, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    start, nodes, g2, p = geometry(name)
    lay = M.seeded_layers(nodes, dtype)
    a, b = M.make(start, dtype, kernel, f64_part), M.make(start, dtype, kernel, f64_part)
    for s in (a, b):
        for l, f in lay.items():
            s.upload_layer(l, f)
    nseg_a = a.update_nodes_shape2d(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"])
    nseg_b = b.update_nodes(nodes)
    ia, ib = a.geometry_info(), b.geometry_info()
    print("shape2d:", ia, "\nnodes:  ", ib)
    assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
    assert nseg_a == nseg_b and ia["segments_z"] > 0
    errs = []
    for step in range(3):
        a.UpdateBoundaries(); b.UpdateBoundaries()
        errs.append((a.TimeStep(dtype(M.DT), 2, 2, True), b.TimeStep(dtype(M.DT), 2, 2, True)))
    print(errs)
    assert all(x == y for x, y in errs)
    assert a.eval_div_error(capi.LAYER_CUR) == b.eval_div_error(capi.LAYER_CUR)
    assert a.last_sweep_kernels() == b.last_sweep_kernels()
    for layer in (capi.LAYER_CUR, capi.LAYER_NEXT):
        for v, (x, y) in enumerate(zip(a.download_layer(layer), b.download_layer(layer))):
            assert np.array_equal(bits(x), bits(y)), "layer %d field %d differs in %d cells" % (layer, v, int((bits(x) != bits(y)).sum()))
    a.close(); b.close()


# ---- 3. the driver -----------------------------------------------------------------------------------------------------------

def test_driver_moving_equals_moving_with_host_extrusion(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("heart_us_2D_data.txt", "heart_us_2D_config.txt"))
    outs = {}
    for word in ("device", "host"):
        prefix = str(tmp_path / word)
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU", "moving"] + (["--host-extrusion"] if word == "host" else []) + ["--steps", "12"],
                           check=True, capture_output=True, text=True, timeout=600, env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
        errs = re.findall(r"err = ([0-9.]+),", r.stdout)
        frames = re.findall(r"frame (\d+)\tsubstep (\d+)", r.stdout)
        n_cs = int(re.search(r"CreateSegments\s+[0-9.]+\s+[0-9.]+\s+(\d+)", r.stdout).group(1))
        outs[word] = (errs, frames, n_cs, open(prefix + "_res.nc", "rb").read())
    print(outs["device"][:3])
    assert len(outs["device"][0]) == 12 and len({f for f, s in outs["device"][1]}) > 1        # the 12 steps cross frame changes
    assert outs["device"][:3] == outs["host"][:3] and outs["device"][2] == 13
    assert len(outs["device"][3]) > 1000 and outs["device"][3] == outs["host"][3]


# ---- 4. allocations ------------------------------------------------------------------------------------------------------------

def test_steady_state_allocates_nothing(built):
    cases = [EC.load_case("heart_us-t3"), EC.load_case("heart_us-t0")]
    s = M.make(cases[1][0], np.float32, capi.SWEEP_AUTO)
    allocs = []
    for r in range(6):
        nodes, g2, p = cases[r % 2]
        s.update_nodes_shape2d(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"])
        allocs.append(s.geometry_info()["device_allocs_and_frees"])
    print("allocs + frees after each update:", allocs)
    assert allocs[0] > 0 and all(x == allocs[1] for x in allocs[1:])
    s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

def small_grid2d(baffle=False):
    """12 x 12 columns authored directly: NODE_OUT ring, NODE_BOUND ring, fluid inside; baffle: a one-cell-thick wall inside the
    fluid, whose middle cells carry a FREE temperature condition and close one X segment while opening the next -- the geometry
    fs3d_upload_nodes refuses (tests/test_gpu_moving.py uses the same one in 3D)."""
    cell = np.full((12, 12), grids.NODE_OUT, np.uint8)
    cell[1:11, 1:11] = grids.NODE_BOUND
    cell[2:10, 2:10] = grids.NODE_IN
    if baffle:
        cell[6, 4:8] = grids.NODE_BOUND
    z = np.zeros((12, 12), np.float32)
    return types.SimpleNamespace(cell=cell, velx=z.copy(), vely=z.copy(), T=np.ones((12, 12), np.float32), dx=0.1, dy=0.1, dimx=12, dimy=12)


SMALL = dict(dz=0.125, depth=1.125, depth_var=0.0, baseT=1.0)      # depth / dz = 9 exactly: active_dimz 10 of dimz 12


def small_nodes(g2):
    return shape2d.extrude_grid2d(g2, SMALL["dz"], SMALL["depth"], SMALL["depth_var"], SMALL["baseT"], dimz=12)


def test_refused_geometry_leaves_no_geometry_until_an_update_succeeds(built):
    good, bad = small_grid2d(), small_grid2d(baffle=True)
    s = M.make(small_nodes(good), np.float32, capi.SWEEP_EXACT)
    with pytest.raises(capi.Fs3dError) as ei:                     # the upload's status for the same nodes ...
        M.make(small_nodes(bad), np.float32, capi.SWEEP_EXACT)
    upload_status = ei.value.status
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes_shape2d(bad, **SMALL)
    assert ei.value.status == upload_status == capi.ERR_UNSUPPORTED and "FREE boundary condition" in str(ei.value)
    for call in (lambda: s.TimeStep(np.float32(M.DT), 1, 1, True), s.UpdateBoundaries, s.geometry_info,
                 lambda: s.clear_outer_cells(capi.LAYER_NEXT, 1.0)):
        with pytest.raises(capi.Fs3dError) as ei:
            call()
        assert ei.value.status == capi.ERR_INVALID and "upload nodes" in str(ei.value)
    s.update_nodes_shape2d(good, **SMALL)
    fresh = M.make(small_nodes(good), np.float32, capi.SWEEP_EXACT)
    ia, ib = s.geometry_info(), fresh.geometry_info()
    assert [ia[k] for k in M.TABLE_KEYS] == [ib[k] for k in M.TABLE_KEYS]
    fresh.upload_layer(capi.LAYER_CUR, s.download_layer(capi.LAYER_CUR))
    for step in range(2):
        s.UpdateBoundaries(); fresh.UpdateBoundaries()
        assert s.TimeStep(np.float32(M.DT), 2, 1, True) == fresh.TimeStep(np.float32(M.DT), 2, 1, True)
    for x, y in zip(s.download_layer(capi.LAYER_CUR), fresh.download_layer(capi.LAYER_CUR)):
        assert np.array_equal(bits(x), bits(y))
    s.close(); fresh.close()


def test_invalid_arguments_are_refused_and_the_context_keeps_its_geometry(built):
    good = small_grid2d()
    s = M.make(small_nodes(good), np.float32, capi.SWEEP_EXACT)
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]

    def refused(g2, **kw):
        with pytest.raises(capi.Fs3dError) as ei:
            s.update_nodes_shape2d(g2, **dict(SMALL, **kw))
        assert ei.value.status == capi.ERR_INVALID, ei.value
        return str(ei.value)

    odd = small_grid2d(); odd.cell[5, 5] = 4
    assert "not a node type" in refused(odd)
    assert "active_dimz" in refused(good, depth=1.5)               # active_dimz 13 > dimz 12
    assert "active_dimz" in refused(good, depth=-0.1)
    assert "active_dimz" in refused(good, dz=0.0)
    assert "bottom" in refused(good, depth_var=50.0)               # the reference's loop would write outside the column
    arrs = s._grid2d_arrays(good)
    nseg = (C.c_int * 3)()
    for hole in range(4):                                          # NULL, each array in turn
        ptrs = [None if q == hole else capi._p(a) for q, a in enumerate(arrs)]
        assert s.lib.fs3d_update_nodes_shape2d(s.h, *ptrs, SMALL["dz"], SMALL["depth"], 0.0, 1.0, nseg) == capi.ERR_INVALID
        assert b"NULL" in s.lib.fs3d_last_error(s.h)
        assert s.lib.fs3d_extrude_shape2d_dev(s.h, *ptrs, SMALL["dz"], SMALL["depth"], 0.0, 1.0, *[None] * 7) == capi.ERR_INVALID
    assert s.lib.fs3d_extrude_shape2d_dev(s.h, *[capi._p(a) for a in arrs], SMALL["dz"], SMALL["depth"], 0.0, 1.0, *[None] * 7) == capi.ERR_INVALID
    # refused before anything was touched: same tables, nothing counted, and the context still steps
    after = s.geometry_info()
    assert [after[k] for k in M.TABLE_KEYS] == [before[k] for k in M.TABLE_KEYS] and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(M.DT), 1, 1, True)
    s.close()


def test_update_before_any_upload_is_invalid(built):
    s = bare_context((12, 12, 12), np.float32)
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes_shape2d(small_grid2d(), **SMALL)
    assert ei.value.status == capi.ERR_INVALID and "fs3d_upload_nodes" in str(ei.value)
    s.close()


def test_update_on_a_slab_context_is_unsupported(built):
    g = grids.box(16, 12, 12)
    s = capi.Solver(g, capi.fluid_params(np.float32, *M.PARAMS), np.float32, x_range=(0, 8))
    g2 = types.SimpleNamespace(cell=np.zeros((16, 12), np.uint8), velx=np.zeros((16, 12), np.float32), vely=np.zeros((16, 12), np.float32),
                               T=np.zeros((16, 12), np.float32))
    nseg = (C.c_int * 3)()
    arrs = [np.ascontiguousarray(g2.cell)] + [np.ascontiguousarray(a) for a in (g2.velx, g2.vely, g2.T)]
    assert s.lib.fs3d_update_nodes_shape2d(s.h, *[capi._p(a) for a in arrs], 0.1, 0.9, 0.0, 1.0, nseg) == capi.ERR_UNSUPPORTED
    assert b"single context" in s.lib.fs3d_last_error(s.h)
    s.UpdateBoundaries()                 # refused before anything was touched: the slab keeps its geometry
    s.close()


# ---- 6. the CreateSegments count ---------------------------------------------------------------------------------------------

def test_create_segments_event_counts_the_updates(built):
    good = small_grid2d()
    s = M.make(small_nodes(good), np.float32, capi.SWEEP_EXACT)
    s.enable_timing(True)
    ms1, n1 = s.profiler_events()["CreateSegments"]
    s.update_nodes_shape2d(good, **SMALL)
    dev_ms = s.last_update_device_ms()
    s.update_nodes_shape2d(good, **dict(SMALL, depth=0.875))
    ms3, n3 = s.profiler_events()["CreateSegments"]
    assert (n1, n3) == (1, 3) and ms3 > ms1 > 0 and dev_ms > 0
    with pytest.raises(capi.Fs3dError):
        s.update_nodes_shape2d(small_grid2d(baffle=True), **SMALL)
    assert s.profiler_events()["CreateSegments"][1] == 3          # a refused geometry is not counted
    s.close()


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "extrude":
        extrude_all_cases(sys.argv[2])
