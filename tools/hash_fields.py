"""sha256 of the fields after one Z sweep with merge and two time steps, on grids that reach every instantiation of the Z partition
kernel, in fp32 and in fp64 (FS3D_OPT_F64_PART on): run it with two builds (FS3D_LIB_PATH) to see whether a kernel change kept
the bits (packed math did, other contractions do not).  python tools/hash_fields.py   (GPU box)"""
import sys, hashlib, numpy as np
sys.path.insert(0, '.')
from cmc_fluid_solver_amd import capi, grids
B, O = grids.box, grids.box_with_obstacle
CASES = {   # Z: lanes per line / waves per line in fp32, fp64
    "box_20x24x28": (lambda: B(20, 24, 28, h=0.04), "f32 f64"),                 # 16, 16
    "obstacle_70x40x36": (lambda: O(70, 40, 36, h=0.02), "f32 f64"),            # 16, 32
    "box_130x100x64": (lambda: B(130, 100, 64, h=0.01), "f32 f64"),             # 16, 32
    "obstacle_9x7x128": (lambda: O(9, 7, 128, h=0.01), "f32 f64"),              # 32, 64
    "obstacle_10x20x256": (lambda: O(10, 20, 256, h=0.004), "f32 f64"),         # 64, pair of waves
    "obstacle_6x9x512": (lambda: O(6, 9, 512, h=0.002), "f32"),                 # pair of waves, full length
    "obstacle_8x10x388": (lambda: O(8, 10, 388, h=0.003), "f32"),               # pair, the upper wave partly past the line
    "box_7x6x260": (lambda: B(7, 6, 260, h=0.004), "f32"),                      # pair, one piece in the upper wave
    "obstacle_8x10x194": (lambda: O(8, 10, 194, h=0.003), "f64"),               # the same two in fp64
    "box_7x6x130": (lambda: B(7, 6, 130, h=0.004), "f64"),
}
for name, (make, dtypes) in CASES.items():
    for tag, dt in (("f32", np.float32), ("f64", np.float64)):
        if tag not in dtypes:
            continue
        g = make()
        s = capi.Solver(g, capi.fluid_params(dt, 200.0, 0.72, 1.4), dt)
        s.set_option(capi.OPT_F64_PART, 1)
        h = hashlib.sha256()
        base = [np.ascontiguousarray(a, dt) for a in (g.vx, g.vy, g.vz, g.T)]
        s.upload_layer(capi.LAYER_CUR, grids.perturb(base, seed=1234)); s.upload_layer(capi.LAYER_TEMP, grids.perturb(base, seed=1235))
        s.sweep(2, 0.1, capi.LAYER_CUR, capi.LAYER_TEMP, capi.LAYER_NEXT, merge=True)
        kz = s.last_sweep_kernels()["Z"]
        for layer in (capi.LAYER_NEXT, capi.LAYER_TEMP):
            for a in s.download_layer(layer): h.update(np.ascontiguousarray(a).tobytes())
        for i in range(2):
            s.UpdateBoundaries(); s.TimeStep(0.1, 2, 2, True)
        for a in s.download_layer(capi.LAYER_CUR): h.update(np.ascontiguousarray(a).tobytes())
        print('HASH', name, tag, h.hexdigest()[:16], 'sweep Z', kz, s.last_sweep_kernels(), flush=True)
        s.close()
