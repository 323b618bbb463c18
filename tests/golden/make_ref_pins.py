#!/usr/bin/env python3
"""Generates tests/golden/ref_pins.npz: what the reference's own pieces (oracle/_ref/libref_pieces.so: Common/Algorithms.h and
Common/Geometry.h; oracle/_ref/libref_config.so: Common/Config.h + LinuxIO.cpp, compiled as they lie by `make -C oracle`) return
on the inputs of the pinned tests in tests/test_oracle_pins.py -- so that those tests hold the oracle and the loaders to the
reference without the reference tree.  When oracle/_ref is built, the tests also check the live library against this file.
Run from the repo root after `make -C oracle`:   python tests/golden/make_ref_pins.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from cmc_fluid_solver_amd import shape2d  # noqa: E402
from oracle import oracle as O  # noqa: E402

INPUTS = os.path.join(HERE, "inputs")
THOMAS_SIZES = (2, 3, 5, 64, 257)
THOMAS_REPS = 5
FP_TRIPLES = ((200.0, 0.72, 1.4), (1000.0, 0.7, 1.3), (50.0, 6.9, 1.01))
FP_PHYSICAL = (0.001, 998.0, 287.0, 0.6, 4180.0)
ALIGN_NS = list(range(0, 200)) + [255, 256, 257, 1023]
CONFIGS = ("box_pipe_2D_config.txt", "non_uniform_pipe_2D_config.txt", "white_sea_config.txt", "heart_us_2D_config.txt")
REJECT_DROP = {"no_vars": "out_vars", "no_dz": "grid_dz", "no_solver": "solver"}
BBOX2D = ("box_pipe_2D_data.txt", "non_uniform_pipe_2D_data.txt", "heart_us_2D_data.txt")
DEPTH_SIZES = ((150, 100), (160, 96), (301, 722), (7, 1000))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def thomas_inputs(dtype):
    """(n, rep, a, b, c, d) of the tridiagonal cases, seeded."""
    rng = np.random.default_rng(1)
    for n in THOMAS_SIZES:
        for rep in range(THOMAS_REPS):
            a = rng.uniform(-1, 1, n).astype(dtype); c = rng.uniform(-1, 1, n).astype(dtype)
            b = rng.uniform(2.1, 4, n).astype(dtype); d = rng.uniform(-5, 5, n).astype(dtype)
            yield n, rep, a, b, c, d


def reject_case(tag):
    good = open(os.path.join(INPUTS, "box_pipe_2D_config.txt")).read().replace("\r", "")
    return "\n".join(ln for ln in good.split("\n") if not ln.startswith(REJECT_DROP[tag]))


def bbox2d_points(name):
    frames = shape2d.parse_shape2d(open(os.path.join(INPUTS, name)).read())
    pts = [np.array([p for sh in fr["shapes"] for p in sh["points"]], np.float32) for fr in frames]
    return len(frames), np.array([len(p) for p in pts], np.int32), np.ascontiguousarray(np.concatenate(pts), np.float32)


def bbox3d_vertices():
    rng = np.random.default_rng(5)
    return [rng.uniform(-30, 50, (40, 3)), rng.uniform(-35, 45, (40, 3))]


def depth_source():
    return np.random.default_rng(6).uniform(-200, 100, (301, 722)).astype(np.float32)


def main():
    import tempfile
    rl = O.ref_lib()
    if rl is None or O.ref_config(os.path.join(INPUTS, CONFIGS[0])) is None:
        sys.exit("oracle/_ref is not built: run `make -C oracle` with the reference tree present")
    out = {}
    for dtype, ct, nm in ((np.float32, C.c_float, "f32"), (np.float64, C.c_double, "f64")):
        for n, rep, a, b, c, d in thomas_inputs(dtype):
            x = np.zeros_like(a)
            getattr(rl, "ref_tridiag_" + nm)(*[v.copy().ctypes.data_as(C.POINTER(ct)) for v in (a, b, c)] +
                                             [d.copy().ctypes.data_as(C.POINTER(ct)), x.ctypes.data_as(C.POINTER(ct))], n)
            out["thomas_%s_%d_%d" % (nm, n, rep)] = x
    pf, pi = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fp = np.zeros((len(FP_TRIPLES), 4), np.float32)
    for k, (Re, Pr, lam) in enumerate(FP_TRIPLES):
        rl.ref_fluid_params_normalized_f32(Re, Pr, lam, fp[k].ctypes.data_as(pf))
    out["fluid_params_normalized_f32"] = fp
    fp = np.zeros(4, np.float32)
    rl.ref_fluid_params_physical_f32(*FP_PHYSICAL, fp.ctypes.data_as(pf))
    out["fluid_params_physical_f32"] = fp
    out["align_by_32"] = np.array([rl.ref_align_by_32(n) for n in ALIGN_NS], np.int32)
    cfg = {name: O.ref_config(os.path.join(INPUTS, name)) for name in CONFIGS}
    with tempfile.TemporaryDirectory() as t:
        for tag in REJECT_DROP:
            p = os.path.join(t, tag + ".txt")
            open(p, "w").write(reject_case(tag))
            cfg[tag] = O.ref_config(p)
    out["config_json"] = np.array(json.dumps(cfg, sort_keys=True))
    for name in BBOX2D:
        nf, npts, xy = bbox2d_points(name)
        bb = np.zeros(4, np.float32)
        rl.ref_bbox2d_build(nf, npts.ctypes.data_as(pi), xy.ctypes.data_as(pf), bb.ctypes.data_as(pf))
        out["bbox2d_" + name] = bb
    # the 3D case goes through shape3d's writer and parser (float32 text): the parsed vertices are the reference's input
    from cmc_fluid_solver_amd import shape3d
    with tempfile.TemporaryDirectory() as t:
        path = os.path.join(t, "m.txt")
        shape3d.write_mesh(path, [(v, np.array([[0, 1, 2]])) for v in bbox3d_vertices()])
        frames = shape3d.parse_shape3d(open(path).read())
    xyz = np.ascontiguousarray(np.concatenate([fr["v"] for fr in frames]), np.float32)
    bb = np.zeros(6, np.float32)
    rl.ref_bbox3d_build(2, np.array([40, 40], np.int32).ctypes.data_as(pi), xyz.ctypes.data_as(pf), bb.ctypes.data_as(pf))
    out["bbox3d_vertices"] = xyz
    out["bbox3d"] = bb
    src = depth_source()
    out["depth_source_sha256"] = np.array(sha(src))
    for nx, ny in DEPTH_SIZES:
        r = np.zeros((nx, ny), np.float32)
        rl.ref_depth_resample(nx, ny, 301, 722, src.ctypes.data_as(pf), r.ctypes.data_as(pf))
        out["depth_%dx%d_sha256" % (nx, ny)] = np.array(sha(r))
    dst = os.path.join(HERE, "ref_pins.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
