"""GPU: the fresh-cell fill (fs3d_fill_fresh_cells_dev, fs3d_fill_fresh_cells; k_fresh_classify, k_fresh_round) against its numpy
twin cmc_fluid_solver_amd/fresh_cells.py bit for bit -- every case of tests/fresh_cells_cases.py, both precisions, two layers, before
and after the layers have swapped buffers -- the snapshot of FS3D_OPT_FRESH_CELLS through every update entry, the allocation
contract, the refusals, the translating sphere against the CPU oracle, and the driver's --fresh-cells.  No tolerance appears."""
import ctypes as C
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

import fresh_cells_cases as FC  # noqa: E402
import mesh_cases as MC  # noqa: E402
import test_gpu_moving as M  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
import watertight_cases as W  # noqa: E402
from test_gpu_extrude import SMALL, small_nodes  # noqa: E402
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, fresh_cells, grids  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits
DTYPES = {"f32": np.float32, "f64": np.float64}
LAYERS = (capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_HALF, capi.LAYER_NEXT)
SEEDS = {capi.LAYER_CUR: 11, capi.LAYER_TEMP: 12, capi.LAYER_NEXT: 14}


def context(nodes, dtype, fresh_option=None):
    s = capi.Solver(nodes, capi.fluid_params(dtype, *M.PARAMS), dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    if fresh_option is not None:
        s.set_option(capi.OPT_FRESH_CELLS, fresh_option)
    return s


def seed_layers(s, size):
    for layer, seed in SEEDS.items():
        s.upload_layer(layer, FC.fields(size, s.dtype.type, seed))


def types_on_device(s, prev_type):
    """The node types as bytes on the context's device without another allocator in the process: packed into field 0 of the HALF
    layer, which no fill writes.  Returns the device pointer."""
    buf = np.zeros(s.dims, s.dtype)
    buf.reshape(-1).view(np.uint8)[:prev_type.size] = np.ascontiguousarray(prev_type, np.uint8).reshape(-1)
    s.upload_layer(capi.LAYER_HALF, [buf, None, None, None])
    p = C.c_void_p()
    s._chk(s.lib.fs3d_field_dev_ptr(s.h, capi.LAYER_HALF, 0, C.byref(p)))
    return p.value


def assert_fields_equal(got, want, what):
    for v, (x, y) in enumerate(zip(got, want)):
        y = np.ascontiguousarray(y, x.dtype)
        assert np.array_equal(bits(x), bits(y)), "%s: field %d differs in %d cells" % (what, v, int((bits(x) != bits(y)).sum()))


def check_fill_dev(s, case, size, ptr, what):
    """fill_fresh_cells_dev on CUR and on NEXT: fields and info equal the twin's, the three other layers keep their bits"""
    for layer in (capi.LAYER_CUR, capi.LAYER_NEXT):
        before = {l: s.download_layer(l) for l in LAYERS}
        info = s.fill_fresh_cells_dev(ptr, layer, FC.MAX_ROUNDS.get(case, 0))
        want, winfo = FC.expected(case, size, s.dtype.type, SEEDS[layer])
        print(what, "layer", layer, "info", info, "twin", winfo)
        assert info == winfo, (what, layer)
        assert_fields_equal(s.download_layer(layer), want, "%s layer %d" % (what, layer))
        for l in LAYERS:
            if l != layer:
                assert_fields_equal(s.download_layer(l), before[l], "%s: untouched layer %d" % (what, l))
        s.upload_layer(layer, before[layer])


# ---- 1, 2. the kernels against the twin, before and after the layers have swapped buffers -----------------------------------------

@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("case", FC.CASES)
def test_fill_equals_the_twin_in_every_layer_slot(built, case, size, prec):
    a, b = FC.pair(case, size)
    s = context(b, DTYPES[prec])
    seed_layers(s, size)
    check_fill_dev(s, case, size, types_on_device(s, a.type), "as created")
    s.UpdateBoundaries()
    s.TimeStep(DTYPES[prec](1e-3), 1, 1, False)             # cur and next have changed buffers
    seed_layers(s, size)
    check_fill_dev(s, case, size, types_on_device(s, a.type), "after a time step")
    s.close()


def test_the_grids_reach_both_paths_of_the_classifying_kernel():
    assert np.prod(FC.SIZES["12x10x16"]) % 8 == 0 and np.prod(FC.SIZES["9x7x11"]) % 8 == 5 and FC.SIZES["9x7x11"][2] % 4 != 0
    # field 0 of a layer begins one halo plane behind an aligned address: 77 cells of 4 bytes are no multiple of 8 (cell by cell),
    # 77 of 8 bytes and 160 of either are (8 cells per thread)
    assert (7 * 11 * 4) % 8 != 0 and (7 * 11 * 8) % 8 == 0 and (10 * 16 * 4) % 8 == 0


# ---- 3. the snapshot of FS3D_OPT_FRESH_CELLS through the update entries ------------------------------------------------------------

def check_snapshot_fill(s, prev_type, type, seed_fields, max_rounds=0):
    s.upload_layer(capi.LAYER_CUR, seed_fields)
    info = s.fill_fresh_cells(capi.LAYER_CUR, max_rounds)
    want, winfo = fresh_cells.fill_fresh_cells(prev_type, type, [np.ascontiguousarray(f, s.dtype) for f in seed_fields], max_rounds)
    print("info", info, "twin", winfo)
    assert info == winfo
    assert_fields_equal(s.download_layer(capi.LAYER_CUR), want, "snapshot fill")
    return info


@pytest.mark.parametrize("size,prec", [("9x7x11", "f32"), ("12x10x16", "f64")])
@pytest.mark.parametrize("case", FC.CASES)
def test_update_nodes_then_fill_equals_the_twin(built, case, size, prec):
    a, b = FC.pair(case, size)
    s = context(a, DTYPES[prec], 1)
    s.update_nodes(b)
    check_snapshot_fill(s, a.type, b.type, FC.fields(size, DTYPES[prec], 11), FC.MAX_ROUNDS.get(case, 0))
    s.close()


def outline(shift):
    """the authored 12 x 12 outline of tests/test_gpu_extrude.py, its walls `shift` columns further along y"""
    cell = np.full((12, 12), grids.NODE_OUT, np.uint8)
    cell[1:11, 1 + shift:10 + shift] = grids.NODE_BOUND
    cell[2:10, 2 + shift:9 + shift] = grids.NODE_IN
    z = np.zeros((12, 12), np.float32)
    return types.SimpleNamespace(cell=cell, velx=z.copy(), vely=z.copy(), T=np.ones((12, 12), np.float32), dx=0.1, dy=0.1, dimx=12, dimy=12)


@pytest.mark.parametrize("prec", list(DTYPES))
def test_update_from_a_moving_outline_then_fill_equals_the_twin(built, prec):
    g0, g1 = outline(0), outline(1)
    n0, n1 = small_nodes(g0), small_nodes(g1)
    s = context(n0, DTYPES[prec], 1)
    s.update_nodes_shape2d(g1, **SMALL)
    rng = np.random.default_rng(5)
    seeded = [np.ascontiguousarray(rng.uniform(-1.0, 1.0, n0.shape) + off, DTYPES[prec]) for off in (0.0, 0.25, -0.5, 1.0)]
    info = check_snapshot_fill(s, n0.type, n1.type, seeded)
    assert info[0] > 0 and info[3] == 0
    s.close()


def sphere_steps(wall_T):
    """WV.translating_grids() with the walls at temperature wall_T"""
    sh, _ = W.sphere(20, (15, 19, 15))
    return [(WV.nodes_of(WV.built(sh, g, idx, vel), wall_T), g, vel, idx) for _, g, vel, idx in WV.translating_grids()]


@pytest.mark.parametrize("prec", list(DTYPES))
def test_update_from_a_moving_mesh_then_fill_equals_the_twin(built, prec):
    steps = sphere_steps(0.0)
    (n3, g3, v3, idx), (n4, g4, v4, _) = steps[3], steps[4]
    s = context(n3, DTYPES[prec], 1)
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    s.update_nodes_shape3d_vel(g4, v4, idx, MC.BASE_T, 0.0)
    rng = np.random.default_rng(6)
    seeded = [np.ascontiguousarray(rng.uniform(-1.0, 1.0, n3.shape) + off, DTYPES[prec]) for off in (0.0, 0.25, -0.5, 1.0)]
    info = check_snapshot_fill(s, n3.type, n4.type, seeded)
    assert info[0] > 100 and info[3] == 0
    s.close()


def child(*args):
    """`python tests/test_gpu_fresh_cells.py <what>` in a fresh process in which torch opens the GPU first"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:], r.stderr[-5000:])
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def device_tensors():
    """update_nodes_dev keeps the snapshot too, and fill_fresh_cells_dev takes a torch tensor: aligned (8 cells per thread) and
    one byte off (cell by cell)"""
    import torch
    case, size = "mixed-origin", "9x7x11"
    a, b = FC.pair(case, size)
    for dtype, td in ((np.float32, torch.float32), (np.float64, torch.float64)):
        s = context(a, dtype, 1)
        ten = [torch.from_numpy(np.ascontiguousarray(x, np.uint8)).cuda() for x in (b.type, b.bc_vel, b.bc_temp)] + \
              [torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda().to(td) for x in (b.vx, b.vy, b.vz, b.T)]
        torch.cuda.synchronize()
        s.update_nodes_dev(*ten)
        check_snapshot_fill(s, a.type, b.type, FC.fields(size, dtype, 11))
        want, winfo = FC.expected(case, size, dtype, 11)
        padded = torch.zeros(a.type.size + 8, dtype=torch.uint8, device="cuda")
        for off in (0, 1):
            prev = padded[off:off + a.type.size]
            prev.copy_(torch.from_numpy(np.ascontiguousarray(a.type, np.uint8).reshape(-1)))
            torch.cuda.synchronize()
            assert prev.data_ptr() % 8 == off
            s.upload_layer(capi.LAYER_CUR, FC.fields(size, dtype, 11))
            assert s.fill_fresh_cells_dev(prev, capi.LAYER_CUR) == winfo
            assert_fields_equal(s.download_layer(capi.LAYER_CUR), want, "tensor at offset %d" % off)
        s.close()
    print("__DEV_OK__")


def test_update_from_device_arrays_keeps_the_snapshot_and_the_fill_takes_tensors(built):
    assert "__DEV_OK__" in child("dev")


def test_the_snapshot_is_valid_only_behind_an_update_of_a_context_that_had_a_geometry(built):
    a, b = FC.pair("one-layer-x", "9x7x11")
    s = context(a, np.float32, 1)

    def refused():
        with pytest.raises(capi.Fs3dError) as ei:
            s.fill_fresh_cells(capi.LAYER_CUR)
        assert ei.value.status == capi.ERR_INVALID, ei.value
        return str(ei.value)
    assert "previous geometry" in refused()                              # no update yet
    s.update_nodes(b)
    assert s.fill_fresh_cells(capi.LAYER_CUR)[0] > 0
    M.upload_nodes(s, a)
    assert "previous geometry" in refused()                              # an upload since
    s.update_nodes(b)
    s.set_option(capi.OPT_FRESH_CELLS, 0)
    assert "FS3D_OPT_FRESH_CELLS" in refused()                           # the option is off
    s.update_nodes(a)                                                    # ... and this update keeps nothing
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    assert "previous geometry" in refused()
    with pytest.raises(capi.Fs3dError):
        s.update_nodes(baffle(a))          # a refused geometry: the context has none
    s.update_nodes(b)                                                    # nothing to take the types from
    assert "previous geometry" in refused()
    s.update_nodes(a)
    assert s.fill_fresh_cells(capi.LAYER_CUR)[0] > 0
    for bad in (2, -1):
        with pytest.raises(capi.Fs3dError) as ei:
            s.set_option(capi.OPT_FRESH_CELLS, bad)
        assert ei.value.status == capi.ERR_INVALID
    s.close()


def baffle(nodes):
    """`nodes` with a one-cell wall of FREE temperature inside the fluid: the geometry the tables refuse"""
    import copy
    g = copy.deepcopy(nodes)
    g.type[2, 2:5, 2:5] = grids.NODE_BOUND
    g.bc_temp[2, 2:5, 2:5] = grids.BC_FREE
    return g


# ---- 4, 5. allocations -------------------------------------------------------------------------------------------------------------

def test_steady_state_allocates_nothing(built):
    a, b = FC.pair("mixed-origin", "12x10x16")
    s = context(a, np.float32, 1)
    allocs = []
    for g in (b, a, b, a):
        s.update_nodes(g)
        s.fill_fresh_cells(capi.LAYER_CUR)
        allocs.append(s.geometry_info()["device_allocs_and_frees"])
    print("allocs + frees after each update and fill:", allocs)
    assert allocs[1] == allocs[2] == allocs[3]


def test_option_off_allocates_what_a_context_without_the_option_does(built):
    a, b = FC.pair("mixed-origin", "12x10x16")
    counts = []
    for option in (None, 0, 1):
        s = context(a, np.float32, option)
        s.update_nodes(b)
        counts.append(s.geometry_info()["device_allocs_and_frees"])
        if option != 1:
            with pytest.raises(capi.Fs3dError) as ei:
                s.fill_fresh_cells(capi.LAYER_CUR)
            assert ei.value.status == capi.ERR_INVALID
            assert s.geometry_info()["device_allocs_and_frees"] == counts[-1]
        s.close()
    assert counts[0] == counts[1] and counts[2] == counts[0] + 1, counts


# ---- 6. the translating sphere against the CPU oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32-exact", "f64-exact"])
def test_translating_sphere_with_the_fill_equals_the_oracle(built, mode):
    dtype, kernel, f64_part = M.MODES[mode]
    O = M._oracle()
    steps = sphere_steps(0.0)
    params = capi.fluid_params(dtype, *M.PARAMS)
    a, b = capi.Solver(steps[0][0], params, dtype), capi.Solver(steps[0][0], params, dtype)        # b: the same run without the fill
    o = O.Oracle(steps[0][0], params, dtype)
    for s in (a, b):
        s.set_option(capi.OPT_SWEEP_KERNEL, kernel); s.set_option(capi.OPT_F64_PART, f64_part); s.set_option(capi.OPT_ERR_ORDER, 1)
        s.set_option(capi.OPT_MESH_VOXELS, 1)
    a.set_option(capi.OPT_FRESH_CELLS, 1)
    prev_type, seen_fresh = steps[0][0].type, False
    for n, (nodes, g, vel, idx) in enumerate(steps):
        for s in (a, b):
            s.update_nodes_shape3d_vel(g, vel, idx, MC.BASE_T, 0.0)
        info = a.fill_fresh_cells(capi.LAYER_CUR)
        o._f("fs3d_oracle_set_nodes")(o.h, *[O._ptr(x) for x in WV.oracle_arrays(nodes, dtype)])
        o._f("fs3d_oracle_create_segments")(o.h)
        filled, winfo = fresh_cells.fill_fresh_cells(prev_type, nodes.type, o.get_layer_fields(O.L_CUR))
        for v in range(4):
            o.set_field(O.L_CUR, v, filled[v])
        print("step", n, "fresh, filled, rounds, left:", info)
        assert info == winfo and info[3] == 0, (n, info, winfo)
        if info[0] and not seen_fresh:                       # directly after the first fill that had something to fill
            seen_fresh = True
            donor, fresh = fresh_cells.classes(prev_type, nodes.type)
            inside = nodes.type == grids.NODE_IN
            Ta, Tb = a.download_layer(capi.LAYER_CUR)[3], b.download_layer(capi.LAYER_CUR)[3]
            print("min T over NODE_IN: with the fill %r, without %r; over the donors %r" % (Ta[inside].min(), Tb[inside].min(), Ta[donor].min()))
            assert Ta[inside].min() >= Ta[donor].min()
            assert (Tb[inside] == 0).any()                   # the defect: fluid cells at exactly the wall's temperature
        for s in (a, b):
            s.UpdateBoundaries()
        ea = a.TimeStep(dtype(WV.RUN_DT), WV.RUN_GL[0], WV.RUN_GL[1], True)
        b.TimeStep(dtype(WV.RUN_DT), WV.RUN_GL[0], WV.RUN_GL[1], False)
        o.update_boundaries()
        rc, eo = o.time_step(float(dtype(WV.RUN_DT)), WV.RUN_GL[0], WV.RUN_GL[1], True)
        M.clear_oracle(o, nodes.type == grids.NODE_OUT, MC.BASE_T)
        assert rc == 0 and eo == ea, (n, eo, ea)
        for s in (a, b):
            s.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); s.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        assert_fields_equal(a.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR), "step %d against the oracle" % n)
        prev_type = nodes.type
    assert seen_fresh
    a.close(); b.close(); o.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

def raw_fill(s, ptr, layer, max_rounds, info=True, dev=True):
    out = (C.c_longlong * 4)()
    args = ([C.c_void_p(ptr) if ptr else None] if dev else []) + [layer, max_rounds, out if info else None]
    st = (s.lib.fs3d_fill_fresh_cells_dev if dev else s.lib.fs3d_fill_fresh_cells)(s.h, *args)
    return st, (s.lib.fs3d_last_error(s.h) or b"").decode()


def test_invalid_arguments_are_refused_and_the_context_is_unchanged(built):
    a, b = FC.pair("mixed-origin", "9x7x11")
    s = context(a, np.float32, 1)
    s.update_nodes(b)
    seed_layers(s, "9x7x11")
    ptr = types_on_device(s, a.type)
    s.fill_fresh_cells(capi.LAYER_NEXT)                                  # the fill's buffers exist from here on
    geom, lay = s.geometry_info(), {l: s.download_layer(l) for l in LAYERS}
    for dev in (True, False):
        for what, kw in (("NULL", dict(info=False)), ("layer", dict(layer=4)), ("layer", dict(layer=-1)), ("max_rounds", dict(max_rounds=251)),
                         ("max_rounds", dict(max_rounds=-1))) + ((("NULL", dict(ptr=0)),) if dev else ()):
            call = dict(dict(ptr=ptr, layer=capi.LAYER_CUR, max_rounds=0, info=True), **kw)
            st, msg = raw_fill(s, call["ptr"], call["layer"], call["max_rounds"], call["info"], dev)
            print(dev, kw, st, msg)
            assert st == capi.ERR_INVALID and what in msg, (dev, kw, st, msg)
            assert s.geometry_info() == geom
            for l in LAYERS:
                assert_fields_equal(s.download_layer(l), lay[l], "layer %d after a refusal" % l)
    want, winfo = FC.expected("mixed-origin", "9x7x11", np.float32, SEEDS[capi.LAYER_CUR])
    assert s.fill_fresh_cells(capi.LAYER_CUR) == winfo                   # and a valid call goes through
    assert_fields_equal(s.download_layer(capi.LAYER_CUR), want, "the valid call")
    s.upload_layer(capi.LAYER_CUR, lay[capi.LAYER_CUR])
    assert s.fill_fresh_cells_dev(ptr, capi.LAYER_CUR) == winfo
    s.close()


def check_slab_refusal(s):
    geom, lay = s.geometry_info(), {l: s.download_layer(l) for l in LAYERS}
    p = C.c_void_p()
    s._chk(s.lib.fs3d_field_dev_ptr(s.h, capi.LAYER_HALF, 0, C.byref(p)))
    for dev in (True, False):
        st, msg = raw_fill(s, p.value, capi.LAYER_CUR, 0, True, dev)
        assert st == capi.ERR_UNSUPPORTED and "single context only" in msg, (dev, st, msg)
    assert s.geometry_info() == geom
    for l in LAYERS:
        assert_fields_equal(s.download_layer(l), lay[l], "layer %d after a refusal" % l)


def test_a_slab_context_and_a_group_member_are_unsupported(built):
    g = grids.box(16, 12, 12)
    s = capi.Solver(g, capi.fluid_params(np.float32, *M.PARAMS), np.float32, x_range=(0, 8))
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    check_slab_refusal(s)
    s.UpdateBoundaries()                                                 # the slab keeps its geometry
    s.close()
    grp = capi.LocalGroup(g, capi.fluid_params(np.float32, *M.PARAMS), 2)
    check_slab_refusal(grp.solvers[1])
    grp.close()


def test_no_nodes_yet_is_invalid(built):
    from test_gpu_extrude import bare_context
    s = bare_context((12, 12, 12), np.float32)
    st, msg = raw_fill(s, 8, capi.LAYER_CUR, 0)                          # (the pointer is never read)
    assert st == capi.ERR_INVALID and "upload nodes first" in msg, (st, msg)
    s.close()


# ---- 8. the driver -----------------------------------------------------------------------------------------------------------------

def test_driver_fresh_cells(built, tmp_path):
    driver = B.build_driver()
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    outs = {}
    for word, extra in (("device", ["moving-mesh", "--watertight", "--fresh-cells"]), ("host", ["moving-mesh", "--host-voxels", "--watertight", "--fresh-cells"]),
                        ("plain", ["moving-mesh", "--watertight"])):
        prefix = str(tmp_path / word)
        r = subprocess.run([driver, data, prefix, cfgf, "align", "GPU"] + extra, check=True, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
        outs[word] = (r.stdout, open(prefix + "_res.nc", "rb").read())
    line = re.search(r"Fresh cells: (\d+) in (\d+) updates, (\d+) filled, at most (\d+) rounds", outs["device"][0])
    print(line and line.group(0))
    assert line and int(line.group(1)) > 0 and int(line.group(2)) in (7, 8) and int(line.group(4)) >= 1
    assert line.group(0) in outs["host"][0] and "Fresh cells:" not in outs["plain"][0]
    assert len(outs["device"][1]) > 1000 and outs["device"][1] == outs["host"][1]
    assert len(outs["plain"][1]) == len(outs["device"][1]) and outs["plain"][1] != outs["device"][1]
    for extra in (["GPU", "2", "--same-device", "moving-mesh", "--host-voxels", "--watertight", "--fresh-cells"], ["GPU", "--watertight", "--fresh-cells"]):
        r = subprocess.run([driver, data, str(tmp_path / "refused"), cfgf, "align"] + extra + ["--steps", "2"], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--fresh-cells:" in r.stderr, (extra, r.returncode, r.stderr)


if __name__ == "__main__":
    import torch
    torch.cuda.init()                    # before the library opens the device
    if sys.argv[1] == "dev":
        device_tensors()
