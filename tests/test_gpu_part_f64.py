"""GPU parity tests of the fp64 partition sweep kernels (FS3D_OPT_F64_PART = 1 on an fp64 context; csrc/kernels_part.hip)
against the CPU oracle and the reference's own fp64 outputs, through the C ABI.

The partition solve and the sequential Thomas recurrence differ by rounding only, so their distance scales with the unit
roundoff.  Every bound below is the bound the project asserts for the same case in fp32 (tests/test_gpu_part.py,
tests/test_gpu_ref_golden.py) x 2^-29 (= eps64 / eps32) x 4; the 4 covers the other chunking of the Z kernel (two cells per
lane, cyclic reduction over up to 128 chunks: up to 3 x in the numpy model, tests/test_f64_part_option.py) and the fp64
reciprocal (v_rcp_f64 + two Newton steps instead of a division).  rel-L2 = ||hip - oracle|| / ||oracle|| over the whole grid.
    one sweep, every field                                               5e-7 (TOL_SWEEP)    -> 3.7e-15
    sweep + merge twice: component of the sweep direction, merged temp   5e-6                -> 3.7e-14
    time steps, velocity as a vector field and T                         1e-6 (TOL_STEPS)    -> 7.5e-15
    small components, of their own norm                                  1e-5                -> 7.5e-14
    reference fixtures                                                   TOL[name]           -> TOL[name] x 7.45e-9
    divergence error                                                     1e-10 relative (what the exact fp64 kernels are held to)
The measured distances are printed (-s) and recorded in DESIGN.md section 5.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import refgolden as RG
from cmc_fluid_solver_amd import capi, grids

pytestmark = pytest.mark.gpu

DT = 0.1
PARAMS = (200.0, 0.72, 1.4)
SCALE = 4.0 * 2.0 ** -29                                   # eps64 / eps32 x 4 = 7.45e-9
# the fp32 constants of tests/test_gpu_part.py: TOL_SWEEP, the 5e-6 of test_sweep_with_merge_within_tolerance, TOL_STEPS, TOL_SMALL_COMPONENT
TOL_SWEEP = 5e-7 * SCALE
TOL_MERGED = 5e-6 * SCALE
TOL_STEPS = 1e-6 * SCALE
TOL_SMALL_COMPONENT = 1e-5 * SCALE
TOL_DIV_ERR = 1e-10
# (velocity, T) of tests/test_gpu_ref_golden.py: TOL
TOL_REF32 = {"u_bend": (1e-6, 1e-6), "box_pipe": (1e-6, 1e-6), "box_pipe_g1l3": (1.7e-6, 1e-6), "box_pipe_g3l1": (1.9e-6, 1e-6),
             "non_uniform_pipe": (1e-6, 1e-6), "box128": (3.4e-6, 1.1e-6), "sphere_3D": (1.8e-6, 5.3e-6)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from oracle import oracle as O
    return O


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def vec_rel(A, B):
    """velocity as a vector field: ||(du, dv, dw)|| / ||(u, v, w)||"""
    num = sum(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2 for a, b in zip(A[:3], B[:3]))
    den = sum(np.linalg.norm(np.asarray(b, np.float64)) ** 2 for b in B[:3])
    return float(np.sqrt(num / max(den, 1e-300)))


def make_pair(g, kernel=capi.SWEEP_PART, fuse=1, f64_part=1):
    O = _oracle()
    params = capi.fluid_params(np.float64, *PARAMS)
    s = capi.Solver(g, params, np.float64)
    s.set_option(capi.OPT_SWEEP_KERNEL, kernel)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    if f64_part is not None:
        s.set_option(capi.OPT_F64_PART, f64_part)
    return s, O.Oracle(g, params, np.float64)


def seed_state(s, o, g, seed=1234):
    O = _oracle()
    base = [np.ascontiguousarray(a, np.float64) for a in (g.vx, g.vy, g.vz, g.T)]
    cur, tmp = grids.perturb(base, seed=seed), grids.perturb(base, seed=seed + 1)
    s.upload_layer(capi.LAYER_CUR, cur); s.upload_layer(capi.LAYER_TEMP, tmp)
    for v in range(4):
        o.set_field(O.L_CUR, v, cur[v]); o.set_field(O.L_TEMP, v, tmp[v])


def assert_step_close(s, o, tol, what):
    O = _oracle()
    A, B = s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR)
    rv, rt = vec_rel(A, B), rel(A[3], B[3])
    print("%s: velocity rel-L2 %.2e, T %.2e, components %s" % (what, rv, rt, ["%.1e" % rel(a, b) for a, b in zip(A[:3], B[:3])]))
    for a in A:
        assert np.isfinite(a).all(), what
    assert rv <= tol and rt <= tol, "%s: velocity rel-L2 %.2e, T rel-L2 %.2e > %.1e" % (what, rv, rt, tol)
    for v in range(3):
        r = rel(A[v], B[v])
        assert r <= TOL_SMALL_COMPONENT, "%s: component %d rel-L2 %.2e of its own norm" % (what, v, r)


# the constructors of the fp32 GRIDS (tests/test_gpu_part.py)
GRIDS = {
    "box_20x24x28": lambda: grids.box(20, 24, 28, h=0.04),
    "obstacle_28x24x32": lambda: grids.box_with_obstacle(28, 24, 32, h=0.03),
    "obstacle_70x40x36": lambda: grids.box_with_obstacle(70, 40, 36, h=0.02),       # lanes past the lane axis, partial chunks; Z: 32 lanes per line, partly used
    "box_130x100x64": lambda: grids.box(130, 100, 64, h=0.01),                      # X: 16 lines x 16 chunks; Z: 32 lanes per line, all used
    "obstacle_256x16x48": lambda: grids.box_with_obstacle(256, 16, 48, h=0.004),     # full-length X lines
    "obstacle_12x256x40": lambda: grids.box_with_obstacle(12, 256, 40, h=0.004),     # full-length Y lines
    "obstacle_10x20x256": lambda: grids.box_with_obstacle(10, 20, 256, h=0.004),     # full-length Z lines: a pair of waves per line
    "obstacle_9x7x128": lambda: grids.box_with_obstacle(9, 7, 128, h=0.01),          # Z: one wave per line, all 64 lanes; odd line count
    # the fp32 grids obstacle_8x10x388 and box_7x6x260 at half the line length: the edge cases of a pair of waves per line
    "obstacle_8x10x194": lambda: grids.box_with_obstacle(8, 10, 194, h=0.003),       # Z: the upper wave partly past the line
    "box_7x6x130": lambda: grids.box(7, 6, 130, h=0.004),                            # Z: one piece in the upper wave
}
SWEEP_GRIDS = ["box_20x24x28", "obstacle_70x40x36", "box_130x100x64", "obstacle_256x16x48", "obstacle_12x256x40", "obstacle_10x20x256", "obstacle_9x7x128",
               "obstacle_8x10x194", "box_7x6x130"]


@pytest.mark.parametrize("gname", SWEEP_GRIDS)
@pytest.mark.parametrize("d", [0, 1, 2])
def test_single_sweep_within_tolerance(built, d, gname):
    """SolveSegments of one direction (AdiSolver3D.cpp:593-603): `next` of every segment cell, nothing else written."""
    O = _oracle()
    g = GRIDS[gname]()
    s, o = make_pair(g)
    assert s.num_segments == [o.num_segments(k) for k in range(3)]
    seed_state(s, o, g)
    sentinel = [np.full(g.shape, 7.25, np.float64) for _ in range(4)]          # cells off the segments must keep it
    s.upload_layer(capi.LAYER_NEXT, sentinel)
    for v in range(4):
        o.set_field(O.L_NEXT, v, sentinel[v])
    s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=False)
    assert s.last_sweep_kernels()["XYZ"[d]] == "part"
    o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT)
    A, B = s.download_layer(capi.LAYER_NEXT), o.get_layer_fields(O.L_NEXT)
    r = [rel(a, b) for a, b in zip(A, B)]
    print("%s sweep %d: rel-L2 per field %s" % (gname, d, ["%.2e" % x for x in r]))
    for v in range(4):
        assert np.isfinite(A[v]).all(), "field %d has non-finite values" % v
        assert r[v] <= TOL_SWEEP, "next after sweep %d: field %d rel-L2 %.2e > %.1e" % (d, v, r[v], TOL_SWEEP)
        assert np.array_equal(A[v] == 7.25, B[v] == 7.25), "the set of written cells differs from the reference's"
    for a, b in zip(s.download_layer(capi.LAYER_TEMP), o.get_layer_fields(O.L_TEMP)):
        assert np.array_equal(a, b), "temp must be untouched by a sweep without merge"
    s.close(); o.close()


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_sweep_with_merge_within_tolerance(built, d, fuse):
    """Sweep + next->MergeLayerTo(temp, NODE_IN) (AdiSolver3D.cpp:651) twice: the second sweep reads the merged temp."""
    O = _oracle()
    g = GRIDS["obstacle_70x40x36"]()
    s, o = make_pair(g, fuse=fuse)
    seed_state(s, o, g)
    for _ in range(2):
        s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        o.sweep(d, DT, O.L_CUR, O.L_TEMP, O.L_NEXT); o.merge(O.L_NEXT, O.L_TEMP)
    assert s.last_sweep_kernels()["XYZ"[d]] == "part"
    A, B = s.download_layer(capi.LAYER_NEXT), o.get_layer_fields(O.L_NEXT)
    T2, U2 = s.download_layer(capi.LAYER_TEMP), o.get_layer_fields(O.L_TEMP)
    print("sweep %d + merge twice (fuse %d): next %s, merged temp %s" % (d, fuse, ["%.2e" % rel(a, b) for a, b in zip(A, B)], ["%.2e" % rel(a, b) for a, b in zip(T2, U2)]))
    for v in range(4):
        # the second sweep reads a merged temp that differs in the last bit of T ~ 1; the momentum row of the sweep direction
        # carries -v_T dT/ds (tests/test_gpu_part.py): that component gets the wider bound
        assert rel(A[v], B[v]) <= (TOL_MERGED if v == d else TOL_SWEEP), "next: field %d rel-L2 %.2e" % (v, rel(A[v], B[v]))
        assert rel(T2[v], U2[v]) <= TOL_MERGED, "merged temp: field %d rel-L2 %.2e" % (v, rel(T2[v], U2[v]))
    notin = g.type != grids.NODE_IN             # cells that are not NODE_IN are copied, not merged: bit-equal
    for a, b in zip(T2, U2):
        assert np.array_equal(a[notin], b[notin])
    s.close(); o.close()


@pytest.mark.parametrize("gname", ["box_20x24x28", "obstacle_28x24x32", "obstacle_70x40x36"])
def test_time_steps_within_tolerance(built, gname):
    """UpdateBoundaries + TimeStep (AdiSolver3D.cpp:286-391), 3 steps, G = 4, L = 2, from the node state, FS3D_SWEEP_AUTO."""
    g = GRIDS[gname]()
    s, o = make_pair(g, capi.SWEEP_AUTO)
    for step in range(3):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, 4, 2, True)
        rc, eo = o.time_step(DT, 4, 2, True)
        print("%s step %d: divergence error %.17g vs %.17g (rel %.1e)" % (gname, step, e, eo, abs(e - eo) / abs(eo)))
        assert rc == 0 and e == pytest.approx(eo, rel=TOL_DIV_ERR)
        assert_step_close(s, o, TOL_STEPS, "%s: cur after step %d" % (gname, step))
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    s.close(); o.close()


@pytest.mark.parametrize("GL", [(1, 1), (2, 1), (1, 3), (3, 2)])
def test_other_iteration_counts(built, GL):
    g = GRIDS["obstacle_28x24x32"]()
    s, o = make_pair(g, capi.SWEEP_AUTO)
    for step in range(2):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, GL[0], GL[1], True); rc, eo = o.time_step(DT, GL[0], GL[1], True)
        assert rc == 0 and e == pytest.approx(eo, rel=TOL_DIV_ERR)
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    assert_step_close(s, o, TOL_STEPS, "G %d L %d: cur" % GL)
    s.close(); o.close()


def test_option_off_is_the_exact_path(built):
    """The default: an fp64 context runs the bit-exact kernels under AUTO and refuses FS3D_SWEEP_PART."""
    O = _oracle()
    g = GRIDS["obstacle_28x24x32"]()
    for setting in (None, 0):                   # never set / set to 0
        s, o = make_pair(g, capi.SWEEP_AUTO, f64_part=setting)
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, 4, 2, True); rc, eo = o.time_step(DT, 4, 2, True)
        assert rc == 0 and e == pytest.approx(eo, rel=TOL_DIV_ERR)
        assert set(s.last_sweep_kernels().values()) == {"pipe"}
        for a, b in zip(s.download_layer(capi.LAYER_CUR), o.get_layer_fields(O.L_CUR)):
            assert np.array_equal(a, b)
        s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_PART)
        for d in range(3):
            with pytest.raises(capi.Fs3dError) as ei:
                s.sweep(d, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
            assert ei.value.status == capi.ERR_UNSUPPORTED
        s.close(); o.close()


def test_fallback_for_one_direction(built):
    """Odd dimz: no whole 16-byte pieces for the Z kernel.  AUTO runs the partition kernels for X and Y and the exact kernel
    for Z; FS3D_SWEEP_PART refuses Z only."""
    g = grids.box(12, 14, 17, h=0.05)
    s, o = make_pair(g, capi.SWEEP_AUTO)
    for step in range(3):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, 4, 2, True); rc, eo = o.time_step(DT, 4, 2, True)
        assert rc == 0 and e == pytest.approx(eo, rel=TOL_DIV_ERR)
    k = s.last_sweep_kernels()
    assert k["X"] == "part" and k["Y"] == "part" and k["Z"] in ("pipe", "line"), k
    assert_step_close(s, o, TOL_STEPS, "12x14x17: cur after 3 steps")
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_PART)
    s.sweep(0, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    s.sweep(1, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    with pytest.raises(capi.Fs3dError) as ei:
        s.sweep(2, DT, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    s.close(); o.close()


def _qualifies(dims):
    return 4 <= dims[0] <= 256 and 4 <= dims[1] <= 256 and 8 <= dims[2] <= 256 and dims[2] % 2 == 0


@pytest.mark.parametrize("name", ["u_bend", "box_pipe", "non_uniform_pipe", "box128", "box_pipe_g1l3", "box_pipe_g3l1", "sphere_3D"])
def test_reference_fixtures_fp64(built, name):
    """The reference's own fp64 outputs (FTYPE double; tests/golden/ref_*_f64.npz): the fixture's arrays where it holds them (full
    fields or the strided sample), the CPU oracle -- bit-equal to the reference there (tests/test_ref_golden.py) -- where it holds
    hashes only (sphere_3D)."""
    fx = RG.Fixture(name, "f64")
    m = fx.meta
    nodes = fx.nodes()
    eng = RG.HipEngine(fx, nodes=nodes)
    eng.s.set_option(capi.OPT_F64_PART, 1)
    ora = RG.OracleEngine(fx, nodes=nodes) if name == "sphere_3D" else None
    ty = fx.z["node_type"]
    worst = [0.0, 0.0]
    st = m["stride"]
    compared = [0]

    class Both:                                 # drives the oracle beside the library where the fixture has no arrays
        def update_boundaries(self):
            eng.update_boundaries()
            if ora:
                ora.update_boundaries()

        def time_step(self, dt, G, L, ce):
            if ora:
                ora.time_step(dt, G, L, ce)
            return eng.time_step(dt, G, L, ce)

        def fields(self):
            return eng.fields()

        def get_layer(self, od):
            if ora:
                ora.get_layer(od)
            return eng.get_layer(od)

    def on_step(step, e):
        got = e.fields()
        if fx.field("U", step) is not None:
            want = [fx.field(v, step) for v in "UVWT"]
            mask = ty != 1
        elif fx.sample("U", step) is not None:
            want = [fx.sample(v, step) for v in "UVWT"]
            got = [a[::st, ::st, ::st] for a in got]
            mask = ty[::st, ::st, ::st] != 1
        elif ora:
            want = ora.fields()
            mask = ty != 1
        else:
            return
        vel = RG.rel_l2(np.stack(got[:3]), np.stack(want[:3]), np.stack([mask] * 3))
        tt = RG.rel_l2(got[3], want[3], mask)
        print("%s f64 step %d: rel-L2 vs the reference  velocity %.3g  T %.3g" % (name, step, vel, tt))
        worst[0], worst[1] = max(worst[0], vel), max(worst[1], tt)
        compared[0] += 1

    try:
        errs = RG.replay(fx, Both(), on_step)
        k = eng.s.last_sweep_kernels()
    finally:
        eng.close()
        if ora:
            ora.close()
    print("%s f64: dims %s, sweep kernels %s, worst velocity %.3g T %.3g" % (name, fx.dims, k, worst[0], worst[1]))
    assert compared[0] > 0
    if name == "u_bend":
        assert fx.dims[2] == 17
        assert k["X"] == "part" and k["Y"] == "part" and k["Z"] in ("pipe", "line"), k     # odd dimz: Z alone falls back
    elif _qualifies(fx.dims):
        assert k == {"X": "part", "Y": "part", "Z": "part"}, k
    else:
        assert "part" in k.values(), k
    assert worst[0] <= TOL_REF32[name][0] * SCALE and worst[1] <= TOL_REF32[name][1] * SCALE, worst
    assert np.allclose(errs, m["err_trace"], rtol=0, atol=6e-9)           # the reference prints %.8f


def test_full_size_256(built):
    """256^3 fp64 box, 2 steps (G 4, L 2) from the node state against the fp64 CPU oracle."""
    g = grids.box(256, h=1.0 / 255)
    s, o = make_pair(g, capi.SWEEP_AUTO)
    for step in range(2):
        s.UpdateBoundaries(); o.update_boundaries()
        e = s.TimeStep(DT, 4, 2, True); rc, eo = o.time_step(DT, 4, 2, True)
        print("256^3 step %d: divergence error %.17g vs %.17g (rel %.1e)" % (step, e, eo, abs(e - eo) / abs(eo)))
        assert rc == 0 and e == pytest.approx(eo, rel=TOL_DIV_ERR)
    assert s.last_sweep_kernels() == {"X": "part", "Y": "part", "Z": "part"}
    assert_step_close(s, o, TOL_STEPS, "256^3 fp64 box after 2 steps")
    s.close(); o.close()


def _sha_fields(fields):
    h = hashlib.sha256()
    for a in fields:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_fp32_context_ignores_the_option(built):
    g = GRIDS["obstacle_70x40x36"]()
    params = capi.fluid_params(np.float32, *PARAMS)
    out = {}
    for on in (0, 1):
        s = capi.Solver(g, params, np.float32)
        s.set_option(capi.OPT_F64_PART, on)
        for i in range(2):
            s.UpdateBoundaries(); s.TimeStep(DT, 4, 2, True)
        out[on] = _sha_fields(s.download_layer(capi.LAYER_CUR)), s.last_sweep_kernels()
        s.close()
    assert out[0] == out[1]
    assert set(out[1][1].values()) == {"part"}


def test_slabs_are_unchanged(built):
    """The option has no effect on slab contexts: a 2-slab in-process group of fp64 contexts under AUTO, 3 steps, with the
    option on every slab context and without -- the same kernels per direction, none of them the partition kernel, and the
    same bits in every field."""
    g = grids.box_with_obstacle(64, 40, 64, h=0.02)
    params = capi.fluid_params(np.float64, *PARAMS)
    out = {}
    for on in (0, 1):
        grp = capi.LocalGroup(g, params, 2, np.float64)

        def steps(r, sv):
            if on:
                sv.set_option(capi.OPT_F64_PART, 1)
            errs = []
            for i in range(3):
                sv.UpdateBoundaries(); errs.append(sv.TimeStep(DT, 4, 2, True))
            return _sha_fields(sv.download_layer(capi.LAYER_CUR)), errs, sv.last_sweep_kernels()
        res = grp.run(steps)
        grp.close()
        for r in res:
            assert all(not v.startswith("part") for v in r[2].values()), r[2]
        out[on] = res
    assert out[0] == out[1], (out[0], out[1])


def test_environment_default_in_a_fresh_process(built):
    """FS3D_DEFAULT_F64_PART=1 sets the option's initial value for new contexts (read in fs3d_create): how bench.py --dtype f64
    and fs3d_run reach the fp64 partition kernels."""
    code = ("import numpy as np\n"
            "from cmc_fluid_solver_amd import capi, grids\n"
            "g = grids.box_with_obstacle(28, 24, 32, h=0.03)\n"
            "s = capi.Solver(g, capi.fluid_params(np.float64, 200.0, 0.72, 1.4), np.float64)\n"
            "s.UpdateBoundaries(); s.TimeStep(0.1, 2, 2, True)\n"
            "print('KERNELS', s.last_sweep_kernels())\n"
            "s.close()\n")
    outs = {}
    for tag, env in (("on", {"FS3D_DEFAULT_F64_PART": "1"}), ("zero", {"FS3D_DEFAULT_F64_PART": "0"})):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=ROOT)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNELS")]
        assert r.returncode == 0 and line, (tag, r.returncode, r.stdout[-300:], r.stderr[-300:])
        outs[tag] = line[0]
    assert outs["on"] == "KERNELS " + str({"X": "part", "Y": "part", "Z": "part"}), outs
    assert outs["zero"] == "KERNELS " + str({"X": "pipe", "Y": "pipe", "Z": "pipe"}), outs
