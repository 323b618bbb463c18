"""GPU: the fresh-cell fill on x-slabs (FS3D_OPT_FRESH_CELLS_SLABS; k_fresh_round<R, true>, fs3d_comm_fill_exchange) -- in-process
groups of 2, 3 and 4 slabs on device 0, the bit-exact kernels, both precisions.  The planes of all ranks together must hold the bits
of the numpy twin's fill of the GLOBAL grid (cmc_fluid_solver_amd/fresh_cells.py); tests/test_fresh_cells_slab_cases.py shows that
a fill which stops at the cuts differs from it on these cases.  No tolerance appears."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import fresh_cells_cases as FC  # noqa: E402
import mesh_cases as MC  # noqa: E402
import test_gpu_moving as M  # noqa: E402
import wall_velocity_cases as WV  # noqa: E402
from test_gpu_fresh_cells import (LAYERS, SEEDS, assert_fields_equal, baffle, raw_fill, sphere_steps,  # noqa: E402
                                  types_on_device)
from cmc_fluid_solver_amd import build as B  # noqa: E402
from cmc_fluid_solver_amd import capi, fresh_cells, grids  # noqa: E402

pytestmark = pytest.mark.gpu

bits = M.bits
DTYPES = {"f32": np.float32, "f64": np.float64}
RANKS = (2, 3, 4)


@pytest.fixture(autouse=True)
def _exact_kernels(monkeypatch):
    """New contexts start on the bit-exact kernels (FS3D_SWEEP_EXACT)."""
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")


def params(dtype):
    return capi.fluid_params(dtype, *M.PARAMS)


def group(nodes, nranks, dtype, fresh=1, slabs=1):
    grp = capi.LocalGroup(nodes, params(dtype), nranks, dtype)
    for s in grp.solvers:
        s.set_option(capi.OPT_FRESH_CELLS, fresh)
        s.set_option(capi.OPT_FRESH_CELLS_SLABS, slabs)
    return grp


@functools.lru_cache(maxsize=None)
def sphere():
    """the translating sphere with walls at T = 0, computed once (the slab threads share it)"""
    return sphere_steps(0.0)


def own(s, a):
    """the planes of the global array `a` that the slab context s owns"""
    return np.ascontiguousarray(a[s.x0:s.x1])


def glue(parts):
    """the four fields of the global grid from every rank's four fields"""
    return [np.concatenate([p[v] for p in parts], axis=0) for v in range(4)]


def check_infos(infos, winfo, what):
    """fresh, filled and left are the ranks' own cells and add up to the twin's; the rounds are the group's on every rank"""
    print(what, "per rank", infos, "twin", winfo)
    for q in (0, 1, 3):
        assert sum(i[q] for i in infos) == winfo[q], (what, q, infos, winfo)
    assert all(i[2] == winfo[2] for i in infos), (what, infos, winfo)
    assert all(i[0] == i[1] + i[3] for i in infos), (what, infos)


# ---- 1. the fields equal the twin's, stateless form --------------------------------------------------------------------------------

def fill_dev_on(case, size, prev_type):
    def work(rank, s):
        out = []
        for step in ("as created", "after a time step"):
            if step != "as created":
                s.UpdateBoundaries()
                s.TimeStep(s.dtype.type(1e-3), 1, 1, False)              # cur and next have changed buffers
            for layer, seed in SEEDS.items():
                s.upload_layer(layer, [own(s, f) for f in FC.fields(size, s.dtype.type, seed)])
            ptr = types_on_device(s, own(s, prev_type))
            for layer in (capi.LAYER_CUR, capi.LAYER_NEXT):
                before = {l: s.download_layer(l) for l in LAYERS}
                info = s.fill_fresh_cells_dev(ptr, layer, FC.MAX_ROUNDS.get(case, 0))
                after = {l: s.download_layer(l) for l in LAYERS}
                s.upload_layer(layer, before[layer])
                out.append((step, layer, info, before, after))
        return out
    return work


@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("size", list(FC.SIZES))
@pytest.mark.parametrize("case", FC.CASES)
def test_fill_on_slabs_equals_the_twin_on_the_global_grid(built, case, size, prec):
    a, b = FC.pair(case, size)
    for nranks in RANKS:
        grp = group(b, nranks, DTYPES[prec])
        res = grp.run(fill_dev_on(case, size, a.type))
        grp.close()
        for n in range(len(res[0])):
            step, layer = res[0][n][0], res[0][n][1]
            what = "%s %s %s, %d ranks, %s, layer %d" % (case, size, prec, nranks, step, layer)
            want, winfo = FC.expected(case, size, DTYPES[prec], SEEDS[layer])
            check_infos([r[n][2] for r in res], winfo, what)
            assert_fields_equal(glue([r[n][4][layer] for r in res]), want, what)
            for r in res:                                                # the other layers' owned planes keep their bits
                for l in LAYERS:
                    if l != layer:
                        assert_fields_equal(r[n][4][l], r[n][3][l], what + ": untouched layer %d" % l)


# ---- 2. the snapshot the slab update entries keep ----------------------------------------------------------------------------------

def refused(s, word, status=capi.ERR_INVALID):
    with pytest.raises(capi.Fs3dError) as ei:
        s.fill_fresh_cells(capi.LAYER_CUR)
    assert ei.value.status == status and word in str(ei.value), ei.value


def snapshot_fill(s, seeded, max_rounds=0):
    s.upload_layer(capi.LAYER_CUR, [own(s, f) for f in seeded])
    info = s.fill_fresh_cells(capi.LAYER_CUR, max_rounds)
    return info, s.download_layer(capi.LAYER_CUR)


@pytest.mark.parametrize("nranks,size,prec", [(2, "9x7x11", "f32"), (3, "12x10x16", "f64"), (4, "9x7x11", "f64")])
@pytest.mark.parametrize("case", ["thick-one", "mixed-origin", "capped", "none"])
def test_update_nodes_slab_then_fill_equals_the_twin(built, case, nranks, size, prec):
    a, b = FC.pair(case, size)
    seeded = FC.fields(size, DTYPES[prec], 11)

    def work(rank, s):
        refused(s, "previous geometry")                                  # no update yet
        s.update_nodes_slab(b)
        return snapshot_fill(s, seeded, FC.MAX_ROUNDS.get(case, 0))
    grp = group(a, nranks, DTYPES[prec])
    res = grp.run(work)
    grp.close()
    want, winfo = FC.expected(case, size, DTYPES[prec], 11)
    check_infos([r[0] for r in res], winfo, "%s %s %d ranks" % (case, size, nranks))
    assert_fields_equal(glue([r[1] for r in res]), want, "snapshot fill")


def test_the_slab_snapshot_follows_the_single_contexts_validity_rules(built):
    a, b = FC.pair("thick-one", "9x7x11")
    seeded = FC.fields("9x7x11", np.float32, 11)

    def work(rank, s):
        refused(s, "previous geometry")                                  # no update yet
        s.update_nodes_slab(b)
        first = snapshot_fill(s, seeded)
        M.upload_nodes(s, a)
        refused(s, "previous geometry")                                  # an upload since
        s.update_nodes_slab(b)
        s.set_option(capi.OPT_FRESH_CELLS, 0)
        refused(s, "FS3D_OPT_FRESH_CELLS")                               # the option is off
        s.update_nodes_slab(a)                                           # ... and this update keeps nothing
        s.set_option(capi.OPT_FRESH_CELLS, 1)
        refused(s, "previous geometry")
        with pytest.raises(capi.Fs3dError):
            s.update_nodes_slab(baffle(b))                               # a refused geometry (a FREE wall cell between two fluid runs of
                                                                         # the global X lines, which every rank reads): the slab has none
        s.update_nodes_slab(a)                                           # nothing to take the types from
        refused(s, "previous geometry")
        s.update_nodes_slab(b)
        return first, snapshot_fill(s, seeded)
    grp = group(a, 3, np.float32)
    res = grp.run(work)
    grp.close()
    want, winfo = FC.expected("thick-one", "9x7x11", np.float32, 11)
    for n in (0, 1):
        check_infos([r[n][0] for r in res], winfo, "fill %d" % n)
        assert_fields_equal(glue([r[n][1] for r in res]), want, "fill %d" % n)


@pytest.mark.parametrize("prec", list(DTYPES))
def test_update_from_a_moving_mesh_on_slabs_then_fill_equals_the_twin(built, prec):
    steps = sphere()
    (n3, g3, v3, idx), (n4, g4, v4, _) = steps[3], steps[4]
    rng = np.random.default_rng(6)
    seeded = [np.ascontiguousarray(rng.uniform(-1.0, 1.0, n3.shape) + off, DTYPES[prec]) for off in (0.0, 0.25, -0.5, 1.0)]
    want, winfo = fresh_cells.fill_fresh_cells(n3.type, n4.type, seeded)
    assert winfo[0] > 100 and winfo[3] == 0

    def work(rank, s):
        s.set_option(capi.OPT_MESH_VOXELS, 1)
        s.update_nodes_shape3d_vel_slab(g4, v4, idx, MC.BASE_T, 0.0)
        return snapshot_fill(s, seeded)
    for nranks in (2, 3):
        grp = group(n3, nranks, DTYPES[prec])
        res = grp.run(work)
        grp.close()
        check_infos([r[0] for r in res], winfo, "sphere step 3 -> 4, %d ranks" % nranks)
        assert_fields_equal(glue([r[1] for r in res]), want, "sphere step 3 -> 4, %d ranks" % nranks)


# ---- 3. the translating sphere: a group against a single context running the same loop ------------------------------------------

def run_sphere(s, dtype, update, fill):
    """every geometry of the translating sphere, walls at T = 0: the update, the fill, a time step, ClearOutterCells on next and cur;
    (cur after every step, the reported errors, the infos of the fills)"""
    s.set_option(capi.OPT_MESH_VOXELS, 1)
    curs, errs, infos = [], [], []
    for nodes, g, vel, idx in sphere():
        update(g, vel, idx, MC.BASE_T, 0.0)
        if fill:
            infos.append(s.fill_fresh_cells(capi.LAYER_CUR))
        s.UpdateBoundaries()
        errs.append(s.TimeStep(dtype(WV.RUN_DT), WV.RUN_GL[0], WV.RUN_GL[1], True))
        s.clear_outer_cells(capi.LAYER_NEXT, MC.BASE_T); s.clear_outer_cells(capi.LAYER_CUR, MC.BASE_T)
        curs.append(s.download_layer(capi.LAYER_CUR))
    return curs, errs, infos


@functools.lru_cache(maxsize=None)
def sphere_single(dtype):
    s = capi.Solver(sphere()[0][0], params(dtype), dtype)
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    out = run_sphere(s, dtype, s.update_nodes_shape3d_vel, True)
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def sphere_group(dtype, nranks, fill):
    grp = group(sphere()[0][0], nranks, dtype, fresh=int(fill), slabs=int(fill))
    res = grp.run(lambda rank, s: run_sphere(s, dtype, s.update_nodes_shape3d_vel_slab, fill))
    grp.close()
    return res


@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("nranks", [2, 3])
def test_translating_sphere_fields_on_slabs_equal_the_single_context(built, nranks, prec):
    dtype = DTYPES[prec]
    ref, _, ref_infos = sphere_single(dtype)
    res = sphere_group(dtype, nranks, True)
    assert sum(i[0] for i in ref_infos) > 0
    for n in range(WV.RUN_STEPS):
        check_infos([r[2][n] for r in res], ref_infos[n], "step %d" % n)
        assert_fields_equal(glue([r[0][n] for r in res]), ref[n], "step %d, %d ranks" % (n, nranks))
    plain = sphere_group(dtype, nranks, False)                           # the same group run without the fill differs
    last = WV.RUN_STEPS - 1
    assert any(not np.array_equal(bits(x), bits(y)) for x, y in zip(glue([r[0][last] for r in plain]), ref[last]))


@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("nranks", [2, 3])
def test_translating_sphere_reported_error_on_slabs_equals_the_single_context(built, nranks, prec):
    """The reported error of every step, on every rank, against the single context's, with `==`: a group adds the per-workgroup
    sums of all global planes in the order a single context adds them (EvalDivError, csrc/fs3d_hip.hip), so equal fields give an
    equal error in both precisions."""
    dtype = DTYPES[prec]
    _, ref_err, _ = sphere_single(dtype)
    res = sphere_group(dtype, nranks, True)
    for r in range(nranks):                                              # every rank holds the global error
        print(nranks, r, [repr(e) for e in res[r][1]], [repr(e) for e in ref_err])
    for r in range(nranks):
        assert res[r][1] == ref_err, (r, res[r][1], ref_err)


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------

def state(s):
    return s.geometry_info(), {l: s.download_layer(l) for l in LAYERS}


def assert_unchanged(s, before, what):
    assert s.geometry_info() == before[0], what
    for l in LAYERS:
        assert_fields_equal(s.download_layer(l), before[1][l], "%s: layer %d" % (what, l))


def test_with_the_option_off_a_group_member_is_refused_as_before(built):
    a, b = FC.pair("thick-one", "12x10x16")

    def work(rank, s):
        s.update_nodes_slab(b)                                           # keeps no snapshot: the slab option is off
        before = state(s)
        p = C.c_void_p()
        s._chk(s.lib.fs3d_field_dev_ptr(s.h, capi.LAYER_HALF, 0, C.byref(p)))
        for dev in (True, False):
            st, msg = raw_fill(s, p.value, capi.LAYER_CUR, 0, True, dev)
            assert st == capi.ERR_UNSUPPORTED and "single context only" in msg, (dev, st, msg)
        assert_unchanged(s, before, "option off")
        for bad in (2, -1):
            with pytest.raises(capi.Fs3dError) as ei:
                s.set_option(capi.OPT_FRESH_CELLS_SLABS, bad)
            assert ei.value.status == capi.ERR_INVALID
        s.set_option(capi.OPT_FRESH_CELLS_SLABS, 1)
        refused(s, "previous geometry")                                  # the update before the option kept nothing
        return True
    grp = group(a, 2, np.float32, fresh=1, slabs=0)
    assert grp.run(work) == [True, True]
    grp.close()


def test_a_lone_slab_needs_its_neighbours(built):
    g = grids.box(16, 12, 12)
    s = capi.Solver(g, params(np.float32), np.float32, x_range=(0, 8))
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    s.set_option(capi.OPT_FRESH_CELLS_SLABS, 1)
    s.update_nodes_slab(g)
    before = state(s)
    p = C.c_void_p()
    s._chk(s.lib.fs3d_field_dev_ptr(s.h, capi.LAYER_HALF, 0, C.byref(p)))
    for dev in (True, False):
        st, msg = raw_fill(s, p.value, capi.LAYER_CUR, 0, True, dev)
        assert st == capi.ERR_UNSUPPORTED and "needs its neighbours" in msg, (dev, st, msg)
    assert_unchanged(s, before, "lone slab")
    s.UpdateBoundaries()                                                 # the slab keeps its geometry
    s.close()


def test_the_option_does_nothing_on_a_single_context(built):
    a, b = FC.pair("mixed-origin", "9x7x11")
    s = capi.Solver(a, params(np.float32), np.float32)
    s.set_option(capi.OPT_FRESH_CELLS, 1)
    s.set_option(capi.OPT_FRESH_CELLS_SLABS, 1)
    s.update_nodes(b)
    s.upload_layer(capi.LAYER_CUR, FC.fields("9x7x11", np.float32, 11))
    want, winfo = FC.expected("mixed-origin", "9x7x11", np.float32, 11)
    assert s.fill_fresh_cells(capi.LAYER_CUR) == winfo
    assert_fields_equal(s.download_layer(capi.LAYER_CUR), want, "single context")
    s.close()


def test_bad_arguments_are_refused_on_every_rank_and_the_slabs_are_unchanged(built):
    """every rank makes the same bad call: each refusal comes before the first word to a peer"""
    a, b = FC.pair("mixed-origin", "9x7x11")
    seeded = FC.fields("9x7x11", np.float32, 11)

    def work(rank, s):
        s.update_nodes_slab(b)
        for layer, seed in SEEDS.items():
            s.upload_layer(layer, [own(s, f) for f in FC.fields("9x7x11", np.float32, seed)])
        ptr = types_on_device(s, own(s, a.type))
        s.fill_fresh_cells(capi.LAYER_NEXT)                              # the fill's buffers exist from here on
        before = state(s)
        for dev in (True, False):
            for what, kw in (("NULL", dict(info=False)), ("layer", dict(layer=4)), ("layer", dict(layer=-1)), ("max_rounds", dict(max_rounds=251)),
                             ("max_rounds", dict(max_rounds=-1))) + ((("NULL", dict(ptr=0)),) if dev else ()):
                call = dict(dict(ptr=ptr, layer=capi.LAYER_CUR, max_rounds=0, info=True), **kw)
                st, msg = raw_fill(s, call["ptr"], call["layer"], call["max_rounds"], call["info"], dev)
                assert st == capi.ERR_INVALID and what in msg, (dev, kw, st, msg)
                assert_unchanged(s, before, "%s %s" % (dev, kw))
        return snapshot_fill(s, seeded)                                  # and a valid call goes through, on all ranks
    grp = group(a, 3, np.float32)
    res = grp.run(work)
    grp.close()
    want, winfo = FC.expected("mixed-origin", "9x7x11", np.float32, 11)
    check_infos([r[0] for r in res], winfo, "the valid call")
    assert_fields_equal(glue([r[1] for r in res]), want, "the valid call")


# ---- 5. allocations ----------------------------------------------------------------------------------------------------------------

def test_steady_state_of_a_group_allocates_nothing(built):
    a, b = FC.pair("thick-one", "12x10x16")

    def work(rank, s):
        allocs = []
        for g in (b, a, b, a):
            s.update_nodes_slab(g)
            s.fill_fresh_cells(capi.LAYER_CUR)
            allocs.append(s.geometry_info()["device_allocs_and_frees"])
        return allocs
    grp = group(a, 4, np.float32)
    res = grp.run(work)
    grp.close()
    print("allocs + frees after each update and fill, per rank:", res)
    for allocs in res:
        assert allocs[0] == allocs[1] == allocs[2] == allocs[3]


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------

FRESH_LINE = r"Fresh cells: (\d+) in (\d+) updates, (\d+) filled, at most (\d+) rounds"


def run_driver(driver, prefix, words):
    data, cfgf = (os.path.join(M.INPUTS, f) for f in ("sphere_3D_data.txt", "sphere_3D_config.txt"))
    r = subprocess.run([driver, data, prefix, cfgf, "align"] + words, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, FS3D_DEFAULT_KERNEL="4"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = re.search(FRESH_LINE, r.stdout)
    return line and line.group(0), re.findall(r"err = ([0-9.]+),", r.stdout), open(prefix + "_res.nc", "rb").read()


@pytest.fixture(scope="module")
def driver(built):
    return B.build_driver()


@pytest.fixture(scope="module")
def driver_single(driver, tmp_path_factory):
    return run_driver(driver, str(tmp_path_factory.mktemp("single") / "one"), ["GPU", "moving-mesh", "--watertight", "--fresh-cells"])


@pytest.mark.parametrize("n", ["2", "3"])
def test_driver_slab_fresh_cells_equals_the_single_gpu_run(driver, driver_single, n, tmp_path):
    got = run_driver(driver, str(tmp_path / "slabs"), ["GPU", n, "--same-device", "moving-mesh", "--slab-voxels", "--watertight", "--slab-fresh-cells"])
    print(driver_single[0], "|", got[0], "|", len(got[1]), "err prints")
    line = re.match(FRESH_LINE, driver_single[0] or "")
    assert line and int(line.group(1)) > 0
    assert got[0] == driver_single[0]
    assert len(got[1]) > 0 and got[1] == driver_single[1]
    assert len(got[2]) > 1000 and got[2] == driver_single[2]


def test_driver_slab_fresh_cells_with_one_gpu_is_fresh_cells(driver, driver_single, tmp_path):
    got = run_driver(driver, str(tmp_path / "one"), ["GPU", "moving-mesh", "--watertight", "--slab-fresh-cells"])
    assert got == driver_single
