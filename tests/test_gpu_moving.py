"""Moving geometry on the GPU: fs3d_update_nodes* rebuilds on the device the tables fs3d_upload_nodes builds on the host, so
everything here is held bit for bit -- to a context that got the same geometry through the upload, and (bit-exact kernels) to
the CPU oracle driven through the same sequence of geometries.  No tolerance is introduced."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:          # run as a script (the child processes below)
    sys.path.insert(0, os.path.dirname(HERE))

import bc_cases  # noqa: E402
import refgolden as RG  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, grids, shape2d  # noqa: E402

pytestmark = pytest.mark.gpu

INPUTS = os.path.join(HERE, "golden", "inputs")
PARAMS = (200.0, 0.72, 1.4)
DT = 0.1
TABLE_KEYS = capi.Solver.GEOMETRY_INFO[:13]        # entry 13 describes the path taken, not the tables
BC_PAIRS = {"bcAB": ("F-A", "F-B"), "bcplates": ("F-C", "P-FN")}


def _oracle():
    from oracle import oracle as O
    return O


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def heart(t):
    fx = RG.Fixture("heart_us", "f32")
    cfg = fx.cfg()
    return shape2d.load_shape2d(fx.data_path, cfg.dx, cfg.dy, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT, fx.meta["align"], time=t)[0]


def heart_case():
    data, cfgf = (os.path.join(INPUTS, f) for f in ("heart_us_2D_data.txt", "heart_us_2D_config.txt"))
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    return data, cfgf, nodes, cfg, dt


def pair(name):
    if name == "box16":
        return grids.box(16, 14, 18), grids.box_with_obstacle(16, 14, 18)
    if name == "box64":
        return grids.box(64), grids.box_with_obstacle(64)
    if name in BC_PAIRS:                               # every FREE / NOSLIP bit of START and END rows in every direction (tests/bc_cases.py)
        return tuple(bc_cases.grid(n) for n in BC_PAIRS[name])
    times = RG.Fixture("heart_us", "f32").meta["grid_times"]
    a, b = {"heart03": (0, 3), "heart45": (4, 5)}[name]
    return heart(times[a]), heart(times[b])


def make(g, dtype, kernel, f64_part=0):
    s = capi.Solver(g, capi.fluid_params(dtype, *PARAMS), dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    s.set_option(capi.OPT_F64_PART, f64_part)
    return s


def upload_nodes(s, nodes):
    """The existing path on a live context: fs3d_upload_nodes again (layers are kept by it too)."""
    arrs = [np.ascontiguousarray(nodes.type, np.uint8), np.ascontiguousarray(nodes.bc_vel, np.uint8),
            np.ascontiguousarray(nodes.bc_temp, np.uint8)] + [np.ascontiguousarray(v, s.dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
    nseg = (C.c_int * 3)()
    s._chk(s.lib.fs3d_upload_nodes(s.h, *[capi._p(a) for a in arrs], nseg))
    return list(nseg)


def seeded_layers(g, dtype):
    base = [np.ascontiguousarray(a, dtype) for a in (g.vx, g.vy, g.vz, g.T)]
    return {capi.LAYER_CUR: grids.perturb(base, seed=1234), capi.LAYER_TEMP: grids.perturb(base, seed=1235),
            capi.LAYER_NEXT: grids.perturb(base, seed=1236)}


def check_update_equals_upload(g1, g2, dtype, kernel, f64_part, dev=False):
    lay = seeded_layers(g2, dtype)
    a = make(g1, dtype, kernel, f64_part)
    for l, f in lay.items():
        a.upload_layer(l, f)
    if dev:
        import torch
        td = torch.float32 if dtype == np.float32 else torch.float64
        ten = [torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() for x in (g2.type, g2.bc_vel, g2.bc_temp)] + \
              [torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda().to(td) for x in (g2.vx, g2.vy, g2.vz, g2.T)]
        torch.cuda.synchronize()
        nseg_a = a.update_nodes_dev(*ten)
    else:
        nseg_a = a.update_nodes(g2)
    b = make(g2, dtype, kernel, f64_part)
    for l, f in lay.items():
        b.upload_layer(l, f)
    ia, ib = a.geometry_info(), b.geometry_info()
    print("update:", ia, "\nupload:", ib)
    assert [ia[k] for k in TABLE_KEYS] == [ib[k] for k in TABLE_KEYS]
    assert nseg_a == b.num_segments
    for step in range(3):
        a.UpdateBoundaries(); b.UpdateBoundaries()
        a.TimeStep(dtype(DT), 2, 2, False); b.TimeStep(dtype(DT), 2, 2, False)
    assert a.eval_div_error(capi.LAYER_CUR) == b.eval_div_error(capi.LAYER_CUR)
    assert a.last_sweep_kernels() == b.last_sweep_kernels()
    for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
        assert np.array_equal(bits(x), bits(y)), "field %d differs in %d cells" % (v, int((bits(x) != bits(y)).sum()))
    a.close(); b.close()


# fp32: the bit-exact kernels and AUTO (the partition kernels); fp64: the bit-exact kernels and AUTO with FS3D_OPT_F64_PART = 1
MODES = {"f32-exact": (np.float32, capi.SWEEP_EXACT, 0), "f32-auto": (np.float32, capi.SWEEP_AUTO, 0),
         "f64-exact": (np.float64, capi.SWEEP_EXACT, 0), "f64-part": (np.float64, capi.SWEEP_AUTO, 1)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["box16", "box64", "heart03", "heart45", "bcAB", "bcplates"])
def test_update_equals_upload(built, name, mode):
    g1, g2 = pair(name)
    check_update_equals_upload(g1, g2, *MODES[mode])


def child(*args):
    """Tests that hand torch tensors to the library run in a fresh process in which torch opens the GPU first (as bench.py does):
    `python tests/test_gpu_moving.py <what> ...`, see the end of this file."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=900)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("mode", ["f32-auto", "f64-exact"])
def test_update_from_device_arrays_equals_upload(built, mode):
    assert "__DEV_OK__" in child("dev", mode)


# ---- a moving run ---------------------------------------------------------------------------------------------------------

def clear_oracle(o, out, baseT):
    O = _oracle()
    for layer in (O.L_NEXT, O.L_CUR):
        for v in range(4):
            f = o.get_field(layer, v)
            f[out] = baseT if v == 3 else 0
            o.set_field(layer, v, f)


def moving_run_vs_oracle(dtype):
    """heart_us through one cycle, a new geometry before every step; the record of what the two engines gave per step."""
    O = _oracle()
    data, cfgf, nodes0, cfg, dt = heart_case()
    params = capi.fluid_params(dtype, cfg.Re, cfg.Pr, cfg.lam)
    s = capi.Solver(nodes0, params, dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    s.set_option(capi.OPT_ERR_ORDER, 1)          # the reported error in the CPU path's summation order: bit-equal too
    o = O.Oracle(nodes0, params, dtype)
    fdt = float(dtype(dt))
    rec = []
    import torch
    torch.cuda.init()
    for n, (t, i, fr, with_err, output) in enumerate(shape2d.time_loop(cfg.grid2d, cfg)):
        nodes = heart(t)
        arrs = [np.ascontiguousarray(nodes.type, np.uint8), np.ascontiguousarray(nodes.bc_vel, np.uint8),
                np.ascontiguousarray(nodes.bc_temp, np.uint8)] + [np.ascontiguousarray(v, dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]
        o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(a) for a in arrs])
        o._f("fs3d_oracle_create_segments")(o.h)
        nseg = s.update_nodes(nodes)
        info = s.geometry_info()
        o.update_boundaries(); s.UpdateBoundaries()
        rc, eo = o.time_step(fdt, cfg.num_global, cfg.num_local, True)
        es = s.TimeStep(dtype(dt), cfg.num_global, cfg.num_local, True)
        lay_ok = True
        if n % 3 == 0:
            (vs, ts), (vo, to) = s.GetLayer(), o.get_layer()
            lay_ok = np.array_equal(bits(vs), bits(vo)) and np.array_equal(ts, to)
        clear_oracle(o, nodes.type == grids.NODE_OUT, cfg.baseT)
        s.clear_outer_cells(capi.LAYER_NEXT, cfg.baseT); s.clear_outer_cells(capi.LAYER_CUR, cfg.baseT)
        diff = [int((bits(a) != bits(b)).sum()) for a, b in zip(s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR))]
        r = dict(step=n, t=float(t), rc=int(rc), err_lib=float(es), err_oracle=float(eo), cells_differing=diff, layer_equal=lay_ok, nseg=nseg,
                 nseg_oracle=[o.num_segments(d) for d in range(3)], allocs=info["device_allocs_and_frees"], bound_cells=info["bound_cells"],
                 mem_free=torch.cuda.mem_get_info()[0])
        print("REC " + json.dumps(r), flush=True)
        rec.append(r)
    s.close(); o.close()
    return rec


def _moving_records(prec):
    return [json.loads(l[4:]) for l in child("moving", prec).splitlines() if l.startswith("REC ")]


@pytest.fixture(scope="module")
def run_f32(built):
    return _moving_records("f32")


@pytest.fixture(scope="module")
def run_f64(built):
    return _moving_records("f64")


def _fields_equal(rec):
    assert len(rec) in (29, 30)
    for r in rec:
        assert r["rc"] == 0 and r["nseg"] == r["nseg_oracle"], r
        assert r["cells_differing"] == [0, 0, 0, 0] and r["layer_equal"], r


def _errors_equal(rec):
    for r in rec:
        assert r["err_lib"] == r["err_oracle"], r


def _errors_small(rec):
    # the oracle alone peaks at 1.5e-7 over this cycle; a missing clear of the NODE_OUT cells shows as >= 1e-3
    for r in rec:
        assert r["err_lib"] < 1e-6 and r["err_oracle"] < 1e-6, r


def test_moving_run_fields_equal_the_cpu_path_f32(run_f32): _fields_equal(run_f32)
def test_moving_run_fields_equal_the_cpu_path_f64(run_f64): _fields_equal(run_f64)
def test_moving_run_error_equals_the_cpu_path_f32(run_f32):
    """The reported error, bit for bit.  The context runs with FS3D_OPT_ERR_ORDER = 1 (EvalDivError sums its per-cell terms in cell
    order, as the CPU path does); with the default parallel summation the fields are bit-identical all the same, the reported
    error differs by up to 2.8e-13 relative (measured over this cycle)."""
    _errors_equal(run_f32)


def test_moving_run_error_equals_the_cpu_path_f64(run_f64):
    _errors_equal(run_f64)


def test_moving_run_error_stays_small_f32(run_f32): _errors_small(run_f32)
def test_moving_run_error_stays_small_f64(run_f64): _errors_small(run_f64)


def test_steady_state_allocates_nothing(run_f32):
    """fs3d_geometry_info entry 13 (device allocations + frees of the geometry paths) after the 3rd and after the last update of
    the cycle.  torch.cuda.mem_get_info is printed, not asserted: the runtime's own pools move it."""
    rec = run_f32
    print("allocs+frees per step:", [r["allocs"] for r in rec])
    print("BOUND/VALVE cells per step:", [r["bound_cells"] for r in rec])
    print("free device memory after update 3 / last: %d / %d bytes" % (rec[2]["mem_free"], rec[-1]["mem_free"]))
    assert rec[2]["allocs"] == rec[-1]["allocs"]
    assert rec[0]["allocs"] > 0


def test_moving_run_auto_kernels_equal_the_upload_path(built):
    """fp32, FS3D_SWEEP_AUTO (partition kernels): the same loop with each geometry through fs3d_update_nodes and, in a second
    context, through fs3d_upload_nodes -- bit for bit, so the partition kernels get no new tolerance."""
    data, cfgf, nodes0, cfg, dt = heart_case()
    params = capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam)
    a, b = capi.Solver(nodes0, params, np.float32), capi.Solver(nodes0, params, np.float32)
    for s in (a, b):
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_AUTO)
    for n, (t, i, fr, with_err, output) in enumerate(shape2d.time_loop(cfg.grid2d, cfg)):
        nodes = heart(t)
        assert a.update_nodes(nodes) == upload_nodes(b, nodes)
        errs = []
        for s in (a, b):
            s.UpdateBoundaries()
            errs.append(s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, True))
            if n % 3 == 0:
                s.GetLayer()
            s.clear_outer_cells(capi.LAYER_NEXT, cfg.baseT); s.clear_outer_cells(capi.LAYER_CUR, cfg.baseT)
        print(n, errs)
        assert errs[0] == errs[1] and errs[0] < 1e-6, (n, errs)
        for v, (x, y) in enumerate(zip(a.download_layer(capi.LAYER_CUR), b.download_layer(capi.LAYER_CUR))):
            assert np.array_equal(bits(x), bits(y)), (n, v)
    assert "part" in a.last_sweep_kernels().values() and a.last_sweep_kernels() == b.last_sweep_kernels()
    a.close(); b.close()


# ---- clear ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_clear_outer_cells(built, dtype):
    g = grids.box_with_obstacle(20, 16, 18)
    s = make(g, dtype, capi.SWEEP_EXACT)
    lay = seeded_layers(g, dtype)
    for l, f in lay.items():
        s.upload_layer(l, f)
    s.UpdateBoundaries()
    s.TimeStep(dtype(DT), 1, 1, True)
    s.GetLayer()
    out = g.type == grids.NODE_OUT
    assert out.any() and (~out).any()
    before = {l: s.download_layer(l) for l in (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF, capi.LAYER_NEXT)}
    for f in before[capi.LAYER_NEXT]:
        assert (f[out] == 99999).all()
    baseT = 1.25
    s.clear_outer_cells(capi.LAYER_NEXT, baseT)
    after = {l: s.download_layer(l) for l in before}
    for v in range(4):
        f = after[capi.LAYER_NEXT][v]
        assert (f[out] == dtype(baseT if v == 3 else 0)).all() and not np.signbit(f[out]).any()
        assert np.array_equal(bits(f)[~out], bits(before[capi.LAYER_NEXT][v])[~out])
        for l in (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF):
            assert np.array_equal(bits(after[l][v]), bits(before[l][v]))
    for bad in (-1, 4):
        with pytest.raises(capi.Fs3dError) as ei:
            s.clear_outer_cells(bad, baseT)
        assert ei.value.status == capi.ERR_INVALID
    s.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------

def baffle_box(n):
    """box(n) with a one-cell-thick baffle across x, temperature BC = FREE: the geometry fs3d_upload_nodes refuses."""
    g = grids.box(n, n, n)
    g.type[n // 2, n // 3:2 * n // 3, n // 3:2 * n // 3] = grids.NODE_BOUND
    g.bc_temp[n // 2, n // 3:2 * n // 3, n // 3:2 * n // 3] = grids.BC_FREE
    return g


def test_refused_geometry_leaves_no_geometry_until_an_update_succeeds(built):
    good = grids.box(12, 12, 12)
    baffle = baffle_box(12)
    other = grids.box_with_obstacle(12, 12, 12)
    s = make(good, np.float32, capi.SWEEP_EXACT)
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes(baffle)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "FREE boundary condition" in str(ei.value)
    for call in (lambda: s.TimeStep(np.float32(DT), 1, 1, True), s.UpdateBoundaries, s.geometry_info,
                 lambda: s.clear_outer_cells(capi.LAYER_NEXT, 1.0)):
        with pytest.raises(capi.Fs3dError) as ei:
            call()
        assert ei.value.status == capi.ERR_INVALID and "upload nodes" in str(ei.value)
    s.update_nodes(other)
    fresh = make(other, np.float32, capi.SWEEP_EXACT)
    fresh.upload_layer(capi.LAYER_CUR, s.download_layer(capi.LAYER_CUR))
    for step in range(2):
        s.UpdateBoundaries(); fresh.UpdateBoundaries()
        assert s.TimeStep(np.float32(DT), 2, 1, True) == fresh.TimeStep(np.float32(DT), 2, 1, True)
    for x, y in zip(s.download_layer(capi.LAYER_CUR), fresh.download_layer(capi.LAYER_CUR)):
        assert np.array_equal(bits(x), bits(y))
    s.close(); fresh.close()


def test_update_before_any_upload_is_invalid(built):
    lib = capi.load()
    h = C.c_void_p()
    assert lib.fs3d_create(C.byref(h), 0, capi.F32, 12, 12, 12, 0.1, 0.1, 0.1, 0, 12) == capi.OK
    g = grids.box(12, 12, 12)
    arrs = [np.ascontiguousarray(a, np.uint8) for a in (g.type, g.bc_vel, g.bc_temp)] + [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    nseg = (C.c_int * 3)()
    try:
        assert lib.fs3d_update_nodes(h, *[capi._p(a) for a in arrs], nseg) == capi.ERR_INVALID
        assert b"fs3d_upload_nodes" in lib.fs3d_last_error(h)
    finally:
        lib.fs3d_destroy(h)


def test_update_on_a_slab_context_is_unsupported(built):
    g = grids.box(16, 12, 12)
    s = capi.Solver(g, capi.fluid_params(np.float32, *PARAMS), np.float32, x_range=(0, 8))
    with pytest.raises(capi.Fs3dError) as ei:
        s.update_nodes(g)
    assert ei.value.status == capi.ERR_UNSUPPORTED and "single context" in str(ei.value)
    s.UpdateBoundaries()                 # refused before anything was touched: the slab keeps its geometry
    s.close()


# The order of the refusals, entry by entry: NULL array, slab, (update entries) no upload yet, the source's own check -- all of
# them before the context gives up its geometry -- and last the refusals of the tables, which leave it without one.
ENTRIES = ["fs3d_update_nodes", "fs3d_update_nodes_dev", "fs3d_update_nodes_shape2d", "fs3d_update_nodes_shape3d",
           "fs3d_extrude_shape2d_dev", "fs3d_voxelize_shape3d_dev", "fs3d_flood_fill_dev"]
SOURCE_OF = {"fs3d_update_nodes_shape2d": "2d", "fs3d_extrude_shape2d_dev": "2d", "fs3d_update_nodes_shape3d": "3d",
             "fs3d_voxelize_shape3d_dev": "3d"}


def raw_entry_call(s, entry, g, null=False, bad_source=False):
    """One call of `entry` on context s with raw ctypes arguments for the 8 x 8 x 8 grid g; null: the first array is NULL;
    bad_source: the Shape2D depth gives active_dimz > dimz, the Shape3D index list names vertex nvert.  Arrays the entry takes
    on the device are fields of the context's own TEMP and HALF layers, so that nothing is handed a pointer it could not use.
    Returns (status, message)."""
    n = g.dimx
    host = [np.ascontiguousarray(a, np.uint8) for a in (g.type, g.bc_vel, g.bc_temp)] + [np.ascontiguousarray(a, np.float32) for a in (g.vx, g.vy, g.vz, g.T)]
    dev = []
    for layer, var in [(capi.LAYER_HALF, v) for v in range(3)] + [(capi.LAYER_TEMP, v) for v in range(4)]:
        p = C.c_void_p()
        s._chk(s.lib.fs3d_field_dev_ptr(s.h, layer, var, C.byref(p)))
        dev.append(p)
    g2 = [np.full((n, n), grids.NODE_IN, np.uint8)] + [np.zeros((n, n), np.float32) for _ in range(3)]
    depth = g.dz * ((n + 1) if bad_source else (n - 2))            # active_dimz = ceil(depth / dz) + 1
    xyz = [np.array(a, np.float32) for a in ([2, 5, 2], [2, 2, 5], [3, 3, 3])]
    tri = np.array([0, 1, 3 if bad_source else 2], np.int32)
    nseg = (C.c_int * 3)()
    hole = lambda ptrs: [None] + ptrs[1:] if null else ptrs
    if entry == "fs3d_update_nodes":
        args = hole([capi._p(a) for a in host]) + [nseg]
    elif entry == "fs3d_update_nodes_dev":
        args = hole(dev) + [nseg]
    elif entry == "fs3d_update_nodes_shape2d":
        args = hole([capi._p(a) for a in g2]) + [g.dz, depth, 0.0, 1.0, nseg]
    elif entry == "fs3d_extrude_shape2d_dev":
        args = hole([capi._p(a) for a in g2]) + [g.dz, depth, 0.0, 1.0] + dev
    elif entry == "fs3d_update_nodes_shape3d":
        args = hole([capi._p(a) for a in xyz]) + [3, capi._p(tri), 1, 1.0, nseg]
    elif entry == "fs3d_voxelize_shape3d_dev":
        args = hole([capi._p(a) for a in xyz]) + [3, capi._p(tri), 1, 1.0] + dev
    else:
        args = hole(dev[:1])
    st = getattr(s.lib, entry)(s.h, *args)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_precedence(built, entry):
    g = grids.box_with_obstacle(8, 8, 8)
    params = capi.fluid_params(np.float32, *PARAMS)
    # a NULL array is named before the slab is
    slab = capi.Solver(g, params, np.float32, x_range=(0, 4))
    st, msg = raw_entry_call(slab, entry, g, null=True)
    print(st, msg)
    assert st == capi.ERR_INVALID and "NULL array" in msg and msg.startswith(entry + ":"), (st, msg)
    st, msg = raw_entry_call(slab, entry, g)
    print(st, msg)
    assert st == capi.ERR_UNSUPPORTED and "single context" in msg and msg.startswith(entry + ":"), (st, msg)
    slab.close()
    # refused by the check of its source, the context keeps the geometry it has
    s = make(g, np.float32, capi.SWEEP_EXACT)
    before = s.geometry_info()
    n_before = s.profiler_events()["CreateSegments"][1]
    if entry in SOURCE_OF:
        st, msg = raw_entry_call(s, entry, g, bad_source=True)
        print(st, msg)
        assert st == capi.ERR_INVALID and msg.startswith(entry + ":"), (st, msg)
        assert ("active_dimz" if SOURCE_OF[entry] == "2d" else "index") in msg, msg
    after = s.geometry_info()
    assert [after[k] for k in TABLE_KEYS] == [before[k] for k in TABLE_KEYS] and s.profiler_events()["CreateSegments"][1] == n_before
    s.UpdateBoundaries(); s.TimeStep(np.float32(DT), 1, 1, True)
    # refused by the tables, it has none
    st, msg = raw_entry_call(s, "fs3d_update_nodes", baffle_box(8))
    print(st, msg)
    assert st == capi.ERR_UNSUPPORTED and "FREE boundary condition" in msg, (st, msg)
    with pytest.raises(capi.Fs3dError) as ei:
        s.geometry_info()
    assert ei.value.status == capi.ERR_INVALID and "upload nodes first" in str(ei.value)
    s.close()


def test_create_segments_event_counts_uploads_and_updates(built):
    g = grids.box(12, 12, 12)
    s = make(g, np.float32, capi.SWEEP_EXACT)
    ms1, n1 = s.profiler_events()["CreateSegments"]
    s.update_nodes(grids.box_with_obstacle(12, 12, 12))
    s.update_nodes(g)
    ms3, n3 = s.profiler_events()["CreateSegments"]
    assert (n1, n3) == (1, 3) and ms3 > ms1 > 0
    s.close()


# ---- the driver -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


def _run_driver(driver, extra, prefix):
    from scipy.io import netcdf_file
    data, cfgf, nodes0, cfg, dt = heart_case()
    out = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + extra + ["--steps", "12"], check=True, capture_output=True, text=True,
                         timeout=600, env=dict(os.environ, FS3D_DEFAULT_KERNEL="4")).stdout
    errs = [float(x) for x in re.findall(r"err = ([0-9.]+),", out)]
    f = netcdf_file(prefix + "_res.nc", "r", mmap=False)
    recs = {v: np.array(f.variables[v][:]) for v in ("u", "v", "w", "T")}
    f.close()
    return out, errs, recs


def _python_loop(moving):
    data, cfgf, nodes0, cfg, dt = heart_case()
    s = capi.Solver(nodes0, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    layers, errs = [], []
    for t, i, fr, with_err, output in shape2d.time_loop(cfg.grid2d, cfg, max_steps=12):
        if moving:
            s.update_nodes(heart(t))
        s.UpdateBoundaries()
        e = s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, with_err)
        errs.append(e if with_err else errs[-1])
        if output:
            layers.append(s.GetLayer((cfg.outdimx, cfg.outdimy, cfg.outdimz)))
        if moving:
            s.clear_outer_cells(capi.LAYER_NEXT, cfg.baseT); s.clear_outer_cells(capi.LAYER_CUR, cfg.baseT)
    s.close()
    return errs, layers


@pytest.mark.parametrize("moving", [True, False])
def test_driver_moving_word(driver, moving, tmp_path):
    """`fs3d_run ... moving`: prints and result records equal the Python loop that moves the geometry through capi; without the
    word the run is the static one (frame 0's geometry throughout), as before."""
    out, errs, recs = _run_driver(driver, ["moving"] if moving else [], str(tmp_path / "heart"))
    ref_err, layers = _python_loop(moving)
    assert len(errs) == 12
    np.testing.assert_allclose(errs, [float("%.8f" % e) for e in ref_err], atol=1e-12)
    assert recs["u"].shape[0] == len(layers)
    for r, (V, T) in enumerate(layers):
        for c, name in enumerate("uvw"):
            np.testing.assert_array_equal(recs[name][r], V[..., c].astype(np.float64))
        np.testing.assert_array_equal(recs["T"][r], T)
    assert ("CreateSegments" in out)
    n_cs = int(re.search(r"CreateSegments\s+[0-9.]+\s+[0-9.]+\s+(\d+)", out).group(1))
    assert n_cs == (13 if moving else 1)


def test_driver_moving_differs_from_static(driver, tmp_path):
    _, e1, r1 = _run_driver(driver, ["moving"], str(tmp_path / "m"))
    _, e0, r0 = _run_driver(driver, [], str(tmp_path / "s"))
    assert not np.array_equal(r1["u"], r0["u"])


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "dev":
        check_update_equals_upload(*pair("heart03"), *MODES[sys.argv[2]], dev=True)
        print("__DEV_OK__")
    elif sys.argv[1] == "moving":
        moving_run_vs_oracle(np.float32 if sys.argv[2] == "f32" else np.float64)
