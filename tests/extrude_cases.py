"""The 2D grids and extrusion parameters that tests/test_extrude_api.py (numpy rule, C++ host function) and
tests/test_gpu_extrude.py (device kernel) are held to.

Shipped inputs: heart_us at the six grid times of its fixture, non_uniform_pipe (depth_var 0.2), u_bend (loaded without
`align`: 53 x 53 x 17, ragged in every axis) and box_pipe.

Degenerate cases on a small authored outline (a passive U closed by two valves, one at rest, one moving): depth / dz giving
active_dimz 2, 3, 4 and 5, each with depth_var 1.0 and 3.0, with and without `align`.  For active_dimz <= 4 the height of the
variable floor is 0 and bottom = 1 everywhere: with active_dimz 2 the floor cell k = 1 lies in the lid and k = 0 is the bound,
with 3 the floor is the bound, with 4 there is no middle.  With active_dimz 5 and depth_var 3.0 bottom reaches
1 + (int)(3 z) <= 4 = active_dimz - 1: the floor passes the bound and enters the lid.  The host function stays inside its arrays
in every one of them (the largest k it writes is max(bottom, active_dimz - 2) < dimz), so none is left out.
"""
import os

import numpy as np

import refgolden as RG
from cmc_fluid_solver_amd import shape2d

HERE = os.path.dirname(os.path.abspath(__file__))

OUTLINE = """1
1.0
3
4
0 12
0 0
10 0
10 12
Passive
2
0 12
5 12
Motion 0 0
2
5 12
10 12
Motion 0 3
"""
OUTLINE_DX = float(np.float32(0.001))   # as a config file gives it (every real number is read through float); the outline is scaled by 0.001 (Grid2D.h:31): 12 x 14 cells
DEGENERATE_DZ = 0.5         # exact in float: depth / dz is an integer, active_dimz = depth / dz + 1


def degenerate_params(adz, depth_var, align):
    return dict(dx=OUTLINE_DX, dy=OUTLINE_DX, dz=DEGENERATE_DZ, depth=DEGENERATE_DZ * (adz - 1), depth_var=depth_var, baseT=1.0, align=align)


DEGENERATE = [("adz%d-var%g-%s" % (a, v, "align" if al else "ragged"), a, v, al) for a in (2, 3, 4, 5) for v in (1.0, 3.0) for al in (True, False)]
SHIPPED = [("heart_us-t%d" % i, "heart_us", i) for i in range(6)] + [(n, n, None) for n in ("non_uniform_pipe", "u_bend", "box_pipe")]
CASE_IDS = [c[0] for c in SHIPPED] + [c[0] for c in DEGENERATE]


def load_case(case_id):
    """(nodes of shape2d.load_shape2d, the Grid2D as it stands at the case's time, params dict for extrude_grid2d)."""
    for cid, name, ti in SHIPPED:
        if cid == case_id:
            fx = RG.Fixture(name, "f32")
            cfg = fx.cfg()
            t = fx.meta["grid_times"][ti] if ti is not None else 0.0
            p = dict(dx=cfg.dx, dy=cfg.dy, dz=cfg.dz, depth=cfg.depth, depth_var=cfg.depth_var, baseT=cfg.baseT, align=fx.meta["align"])
            nodes, g2 = shape2d.load_shape2d(fx.data_path, p["dx"], p["dy"], p["dz"], p["depth"], p["depth_var"], p["baseT"], p["align"], time=t)
            return nodes, g2, p
    for cid, adz, var, align in DEGENERATE:
        if cid == case_id:
            p = degenerate_params(adz, var, align)
            nodes, g2 = shape2d.load_shape2d(OUTLINE, p["dx"], p["dy"], p["dz"], p["depth"], p["depth_var"], p["baseT"], p["align"], is_text=True)
            assert shape2d.active_dimz_of(p["dz"], p["depth"]) == adz
            return nodes, g2, p
    raise KeyError(case_id)


def twin(g2, p):
    return shape2d.extrude_grid2d(g2, p["dz"], p["depth"], p["depth_var"], p["baseT"], p["align"])


NODE_ARRAYS = ("type", "bc_vel", "bc_temp", "vx", "vy", "vz", "T")


def assert_nodes_equal(a, b):
    assert tuple(a.shape) == tuple(b.shape)
    for name in NODE_ARRAYS:
        x, y = np.ascontiguousarray(getattr(a, name)), np.ascontiguousarray(getattr(b, name))
        assert x.dtype == y.dtype, name
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s differs in %d cells" % (name, int((x != y).sum()))


def config_text(p):
    """A driver config for the authored outline (host/Config.h reads every real number through float; baseT is its constant 1.0)."""
    return ("dimension 3D\nin_fmt Shape2D\ndepth %r\ndepth_var %r\nRe 200.0\nPr 0.72\nlambda 1.4\nbc_type NoSlip\n"
            "grid_dx %r\ngrid_dy %r\ngrid_dz %r\ncycles 1\ntime_steps 10\nout_fmt NetCDF\nout_time_steps 5\nout_gridx 6\nout_gridy 6\n"
            "out_gridz 2\nout_vars 4 u v w T\nsolver ADI\nnum_global 2\nnum_local 1\n" % (p["depth"], p["depth_var"], p["dx"], p["dy"], p["dz"]))
