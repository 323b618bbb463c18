"""ctypes binding of libfs3d_hip.so (include/fs3d.h) and a thin `Solver` class that
mirrors the reference's Solver3D / AdiSolver3D host interface
(Solver3D.h:24-49, AdiSolver3D.h:61-70): Init / UpdateBoundaries / TimeStep / GetLayer.

There is NO fallback: if the HIP library is missing or no GPU is present the calls
fail loudly (RuntimeError carrying fs3d_last_error()).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FS3D_LIB_PATH") or os.path.join(_HERE, "libfs3d_hip.so")   # override: kernel experiments

F32, F64 = 0, 1
OK, ERR_INVALID, ERR_HIP, ERR_DIVERGED, ERR_UNSUPPORTED, ERR_COMM = range(6)
DIR_X, DIR_Y, DIR_Z = 0, 1, 2
LAYER_CUR, LAYER_TEMP, LAYER_HALF, LAYER_NEXT = 0, 1, 2, 3
SWEEP_AUTO, SWEEP_LINE, SWEEP_PIPE, SWEEP_PART, SWEEP_EXACT = 0, 1, 2, 3, 4
KERNEL_NAMES = {0: "none", 1: "line", 2: "pipe", 3: "part"}
OPT_SWEEP_KERNEL, OPT_FUSE_MERGE, OPT_DIV_CORE, OPT_XSOLVE, OPT_OVERLAP, OPT_KEEP_TEMP = 0, 1, 2, 3, 4, 5
OPT_F64_PART = 6          # fp64 contexts: 1 opens the fp64 partition kernels to SWEEP_AUTO / SWEEP_PART (default 0: bit-exact kernels)
OPT_ERR_ORDER = 7         # 1: EvalDivError sums its terms serially in cell order, as the CPU path (bit-equal reported error on the exact kernels)
OPT_MESH_VOXELS = 8       # the two mesh entries: 0 the reference's rasteriser (default), 1 conservative voxelisation (watertight)
MESH_VOXELS = {"reference": 0, "conservative": 1}
OPT_FRESH_CELLS = 9       # 1: every single-context update_nodes* keeps the node types of the geometry it replaces, for fill_fresh_cells (default 0)
OPT_MESH_SHELL = 11       # the mesh entries, with the conservative voxelisation: 0 every cell whose box a triangle touches (default), 1 the thin shell
MESH_SHELL = {"box": 0, "cross": 1}
OPT_FRESH_CELLS_SLABS = 10  # 1: a slab of a group keeps that snapshot too (the update_nodes*_slab entries) and fill_fresh_cells* run collectively (default 0)
OPT_OUTPUT_FILTER = 12    # the three GetLayer entries: 0 the reference's point sample (default), 1 the mean over the NODE_IN cells of the sample's box
OUTPUT_FILTER = {"point": 0, "box": 1}
OPT_OUTPUT_VECTOR = 13    # outV of the same entries: 0 the velocity (default), 1 the vorticity (layer_output.py is the rule of both options)
OUTPUT_VECTOR = {"velocity": 0, "vorticity": 1}
OPT_TIME_STATS = 14       # 1: every successful time step adds the new `cur` to per-cell sums on the device, 2: and its squares; every set opens a new window (default 0)
TIME_STATS = {"off": 0, "mean": 1, "variance": 2}
OPT_OUTPUT_SOURCE = 15    # what the three GetLayer entries sample: 0 `next` (default), 1 the time mean, 2 the time variance, 3 the fluid fraction (time_stats.py is the rule)
OUTPUT_SOURCE = {"next": 0, "mean": 1, "variance": 2, "fraction": 3}
OPT_TIME_STATS_CROSS = 16  # 1: mode 2 also sums the six products uv, uw, vw, uT, vT, wT per cell; every set opens a new window, 0 frees them (default 0)
OPT_OUTPUT_MOMENT = 17    # what source 2 builds: 0 the variances (default), 1 the Reynolds stresses and k, 2 the heat fluxes and var_T (time_stats.MOMENTS)
OPT_TIME_STATS_EVERY = 18  # the stride k of the accumulated steps, 1 (default) .. 2^20: candidate s of a window counts where (s - 1) % k == 0; every set opens a new window
OPT_OUTPUT_SLABS = 19     # 1: on a member of a group GetLayerRows / GetLayerDev take the filter and vector options, as one collective call (default 0)
OPT_OUTPUT_GRADIENT = 20  # outV of the three GetLayer entries: 0 as FS3D_OPT_OUTPUT_VECTOR has it (default), 1 the invariants (div, Q, S:S) of the velocity gradient of the
                          # sampled layer, 2 their time mean from the gradient sums (layer_output.invariants, time_stats.TimeStats.gradient_layer are the rule)
OPT_TIME_STATS_GRAD = 21  # 1: every accumulated step also sums div, Q and S:S of the new `cur` per cell; whole grids only; every set opens a new window, 0 frees them (default 0)
OPT_OUTPUT_WALL = 22      # outV of the three GetLayer entries: 0 as the options above have it (default), 1 the wall shear stress tau of the sampled layer on the wall cells that
                          # carry one, 2 (|tau|, the wall heat flux q, the exposed area), 3 the time mean of tau, 4 (tawss, mean q, osi) from the wall sums
                          # (layer_output.wall_loads, time_stats.TimeStats.wall_layer are the rule); whole grids only
OPT_TIME_STATS_WALL = 23  # 1: every accumulated step also sums tau, |tau| and q of the new `cur` per carrier; whole grids only; every set opens a new window, 0 frees them (default 0)
XSOLVE_AUTO, XSOLVE_PIPELINED, XSOLVE_REDUCED, XSOLVE_REDUCED_A2A = 0, 1, 2, 3

# every function include/fs3d.h declares, in the header's order: name -> (restype, argtypes)
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_pi, _pll, _pf = C.POINTER(_i), C.POINTER(C.c_longlong), C.POINTER(C.c_float)
_nodes, _grid2d = [_vp] * 7, [_vp] * 4 + [_d] * 4        # the seven SoA node arrays; cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT
_mesh, _mesh_vel = [_vp] * 3 + [_i, _vp, _i, _d], [_vp] * 6 + [_i, _vp, _i, _d, _d]     # x, y, z[, wx, wy, wz], nvert, tri, ntri, baseT[, wallT]
N_EVENTS = 9              # FS3D_N_EVENTS: the length of the three arrays of fs3d_profiler_events
SYMBOLS = {
    "fs3d_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _i, _d, _d, _d, _i, _i]),
    "fs3d_destroy": (None, [_vp]),
    "fs3d_last_error": (C.c_char_p, [_vp]),
    "fs3d_set_params": (_i, [_vp, _d, _d, _d, _d]),
    "fs3d_set_option": (_i, [_vp, _i, _i]),
    "fs3d_upload_nodes": (_i, [_vp] + _nodes + [_pi]),
    "fs3d_update_nodes": (_i, [_vp] + _nodes + [_pi]),
    "fs3d_update_nodes_dev": (_i, [_vp] + _nodes + [_pi]),
    "fs3d_update_nodes_slab": (_i, [_vp] + _nodes + [_pi]),
    "fs3d_extrude_shape2d_dev": (_i, [_vp] + _grid2d + _nodes),
    "fs3d_update_nodes_shape2d": (_i, [_vp] + _grid2d + [_pi]),
    "fs3d_update_nodes_shape2d_slab": (_i, [_vp] + _grid2d + [_pi]),
    "fs3d_shape2d_bottom": (_i, [_i, _i, _d, _d, _d, _pi]),
    "fs3d_update_nodes_shape3d": (_i, [_vp] + _mesh + [_pi]),
    "fs3d_update_nodes_shape3d_vel": (_i, [_vp] + _mesh_vel + [_pi]),
    "fs3d_update_nodes_shape3d_slab": (_i, [_vp] + _mesh + [_pi]),
    "fs3d_update_nodes_shape3d_vel_slab": (_i, [_vp] + _mesh_vel + [_pi]),
    "fs3d_voxelize_shape3d_dev": (_i, [_vp] + _mesh + _nodes),
    "fs3d_voxelize_shape3d_vel_dev": (_i, [_vp] + _mesh_vel + _nodes),
    "fs3d_flood_fill_dev": (_i, [_vp, _vp]),
    "fs3d_flood_fill_global_dev": (_i, [_vp, _vp]),
    "fs3d_mesh_fill_rounds": (_i, [_vp, _pi]),
    "fs3d_fill_fresh_cells_dev": (_i, [_vp, _vp, _i, _i, _pll]),
    "fs3d_fill_fresh_cells": (_i, [_vp, _i, _i, _pll]),
    "fs3d_last_fill_device_ms": (_i, [_vp, _pf]),
    "fs3d_clear_outer_cells": (_i, [_vp, _i, _d]),
    "fs3d_last_update_device_ms": (_i, [_vp, _pf]),
    "fs3d_geometry_info": (_i, [_vp, _pll]),
    "fs3d_geometry_dead_lines": (_i, [_vp, _i, _vp, _pll]),
    "fs3d_init_layers_from_nodes": (_i, [_vp]),
    "fs3d_upload_layer": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "fs3d_download_layer": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "fs3d_field_dev_ptr": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "fs3d_update_boundaries": (_i, [_vp]),
    "fs3d_time_step": (_i, [_vp, _d, _i, _i, _i, C.POINTER(_d)]),
    "fs3d_time_step_async": (_i, [_vp, _d, _i, _i]),
    "fs3d_synchronize": (_i, [_vp]),
    "fs3d_sweep": (_i, [_vp, _i, _d, _i, _i, _i, _i]),
    "fs3d_merge": (_i, [_vp, _i, _i]),
    "fs3d_eval_div_error": (_i, [_vp, _i, C.POINTER(_d), _pll]),
    "fs3d_get_layer": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "fs3d_get_layer_rows": (_i, [_vp, _vp, _vp, _i, _i, _i, _pi]),
    "fs3d_get_layer_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _pi]),
    "fs3d_get_layer_info": (_i, [_vp, _pll]),
    "fs3d_comm_unique_id": (_i, [_vp]),
    "fs3d_comm_init": (_i, [_vp, _vp, _i, _i]),
    "fs3d_local_group_create": (_i, [_i, C.POINTER(_vp)]),
    "fs3d_local_group_destroy": (None, [_vp]),
    "fs3d_local_group_abort": (None, [_vp]),
    "fs3d_comm_init_local": (_i, [_vp, _vp, _i]),
    "fs3d_comm_abort": (_i, [_vp]),
    "fs3d_comm_selftest": (_i, [_vp, C.c_size_t]),
    "fs3d_last_step_timing": (_i, [_vp, _pf, _pi]),
    "fs3d_profiler_events": (_i, [_vp, C.POINTER(C.c_char_p), _pf, _pi]),
    "fs3d_enable_timing": (_i, [_vp, _i]),
    "fs3d_profile_sweep": (_i, [_vp, _i, _d, _i, _i, _i, C.POINTER(C.c_ulonglong), _i, _pi]),
    "fs3d_last_sweep_kernel": (_i, [_vp, _i, _pi, _pi]),
    "fs3d_last_sweep_launch": (_i, [_vp, _i, _i, _pi]),
    "fs3d_version": (C.c_char_p, []),
}

_lib = None


class Fs3dError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("fs3d status %d: %s" % (status, msg))
        self.status = status


def load():
    """dlopen libfs3d_hip.so and bind every declared symbol.  No GPU is touched."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libfs3d_hip.so is not built (%s); run `python -m cmc_fluid_solver_amd.build` "
                               "or __graft_entry__.build()" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Solver:
    """Host-side mirror of the reference's AdiSolver3D for ONE GPU / one x-slab.

    Init(grid, params) -> __init__(nodes, params) ; UpdateBoundaries ; TimeStep ; GetLayer.
    `nodes` is the GLOBAL grids.Nodes object; x_range selects the owned planes.
    """

    def __init__(self, nodes, params, dtype=np.float32, device=0, x_range=None):
        self.lib = load()
        self.dtype = np.dtype(dtype)
        self.prec = F32 if self.dtype == np.float32 else F64
        x0, x1 = x_range if x_range is not None else (0, nodes.dimx)
        self.x0, self.x1 = x0, x1
        self.dims = (x1 - x0, nodes.dimy, nodes.dimz)
        self.gdims = nodes.shape
        self.h = C.c_void_p()
        st = self.lib.fs3d_create(C.byref(self.h), device, self.prec, x1 - x0, nodes.dimy, nodes.dimz,
                                  nodes.dx, nodes.dy, nodes.dz, x0, nodes.dimx)
        if st != OK:
            raise Fs3dError(st, (self.lib.fs3d_last_error(None) or b"").decode())
        self._chk(self.lib.fs3d_set_params(self.h, *[float(p) for p in params]))
        self._update(self.lib.fs3d_upload_nodes, *[_p(a) for a in self._node_arrays(nodes)])
        self._chk(self.lib.fs3d_init_layers_from_nodes(self.h))

    # -- plumbing -----------------------------------------------------------------
    def _chk(self, st):
        if st != OK:
            raise Fs3dError(st, (self.lib.fs3d_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.fs3d_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt, val):
        self._chk(self.lib.fs3d_set_option(self.h, opt, val))

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.lib.fs3d_comm_init(self.h, buf, rank, nranks))

    def comm_selftest(self, elems=1 << 18):
        """One-rank RCCL communicator on this context's device: grouped send/recv, all-gather, all-reduce, verified."""
        self._chk(self.lib.fs3d_comm_selftest(self.h, elems))

    def comm_abort(self):
        self._chk(self.lib.fs3d_comm_abort(self.h))

    def comm_init_local(self, group, rank):
        self._chk(self.lib.fs3d_comm_init_local(self.h, group.h, rank))
        self._group = group        # keep the group alive as long as the context

    # -- moving geometry ------------------------------------------------------------
    def _node_arrays(self, nodes):
        """The seven node arrays as the C ABI takes them from the host: uint8 x 3, the context's precision x 4."""
        return [np.ascontiguousarray(a, np.uint8) for a in (nodes.type, nodes.bc_vel, nodes.bc_temp)] + [
            np.ascontiguousarray(v, self.dtype) for v in (nodes.vx, nodes.vy, nodes.vz, nodes.T)]

    def _update(self, fn, *args):
        """fn(ctx, *args, n_seg_out): an entry that leaves the context with new tables; sets and returns num_segments."""
        nseg = (C.c_int * 3)()
        self._chk(fn(self.h, *args, nseg))
        self.num_segments = list(nseg)
        return self.num_segments

    def _dev_ptrs(self, what, arrays):
        """Node arrays on the context's device (the byte arrays first) as pointers; `what` names the method in the refusal."""
        def ptr(a, want):
            if isinstance(a, int):
                return C.c_void_p(a)
            if not a.is_cuda or not a.is_contiguous() or a.element_size() != want or a.numel() != int(np.prod(self.gdims)):
                raise ValueError(what + ": contiguous device tensors of the grid's size and the context's precision")
            return C.c_void_p(a.data_ptr())
        return [ptr(a, 1) for a in arrays[:3]] + [ptr(a, self.dtype.itemsize) for a in arrays[3:]]

    def _update_arrays(self, fn, nodes):
        assert tuple(nodes.shape) == tuple(self.gdims)
        return self._update(fn, *[_p(a) for a in self._node_arrays(nodes)])

    def update_nodes(self, nodes):
        """AdiSolver3D::CreateSegments between time steps: the tables of a new geometry (same dims), rebuilt on the device.
        Layers are kept.  After a refusal the context has no geometry until an update succeeds."""
        return self._update_arrays(self.lib.fs3d_update_nodes, nodes)

    def update_nodes_slab(self, nodes):
        """update_nodes on an x-slab (or a whole-grid context): `nodes` is the GLOBAL grid, every rank of a group is given the
        same one between the same two steps and rebuilds the tables of its own planes; no rank waits for another."""
        return self._update_arrays(self.lib.fs3d_update_nodes_slab, nodes)

    def update_nodes_dev(self, type, bc_vel, bc_temp, vx, vy, vz, T):
        """The same from arrays on the context's device: torch tensors (contiguous; uint8 x 3, the context's precision x 4)
        or raw device pointers (int)."""
        return self._update(self.lib.fs3d_update_nodes_dev, *self._dev_ptrs("update_nodes_dev", [type, bc_vel, bc_temp, vx, vy, vz, T]))

    def _grid2d_arrays(self, g2):
        """cell, velx, vely, T of a shape2d.Grid2D (or any object with these four [dimx, dimy] arrays) as the C ABI takes them."""
        arrs = [np.ascontiguousarray(g2.cell, np.uint8)] + [np.ascontiguousarray(a, np.float32) for a in (g2.velx, g2.vely, g2.T)]
        for a in arrs:
            if a.shape != tuple(self.gdims[:2]):
                raise ValueError("the 2D grid is %s, the context's plane %s" % (a.shape, tuple(self.gdims[:2])))
        return arrs

    def extrude_shape2d_dev(self, g2, dz, depth, depth_var, baseT, type, bc_vel, bc_temp, vx, vy, vz, T):
        """Grid3D::Prepare2D on the device: the 2D grid g2 as it stands (after g2.prepare(t)) extruded into seven arrays on the
        context's device -- torch tensors or raw pointers, as update_nodes_dev takes them.  The context's geometry is not touched."""
        ptrs = self._dev_ptrs("extrude_shape2d_dev", [type, bc_vel, bc_temp, vx, vy, vz, T])
        arrs = self._grid2d_arrays(g2)
        self._chk(self.lib.fs3d_extrude_shape2d_dev(self.h, *[_p(a) for a in arrs], float(dz), float(depth), float(depth_var), float(baseT), *ptrs))

    def _update_shape2d(self, fn, g2, dz, depth, depth_var, baseT):
        arrs = self._grid2d_arrays(g2)
        return self._update(fn, *[_p(a) for a in arrs], float(dz), float(depth), float(depth_var), float(baseT))

    def update_nodes_shape2d(self, g2, dz, depth, depth_var, baseT):
        """update_nodes with the extrusion of the 2D grid g2 as the source: 13 bytes per column travel, the node arrays are written
        by a kernel.  Same contract as update_nodes."""
        return self._update_shape2d(self.lib.fs3d_update_nodes_shape2d, g2, dz, depth, depth_var, baseT)

    def update_nodes_shape2d_slab(self, g2, dz, depth, depth_var, baseT):
        """update_nodes_shape2d on an x-slab (or a whole-grid context): g2 is the GLOBAL 2D grid, given to every rank."""
        return self._update_shape2d(self.lib.fs3d_update_nodes_shape2d_slab, g2, dz, depth, depth_var, baseT)

    @staticmethod
    def _mesh_arrays(g, idx):
        """x, y, z (float32) and the flat index list (int32) of vertices g [n, 3] in grid coordinates and triangles idx [m, 3]."""
        g = np.asarray(g, np.float32).reshape(-1, 3)
        xyz = [np.ascontiguousarray(g[:, a]) for a in range(3)]
        tri = np.ascontiguousarray(np.asarray(idx).reshape(-1), np.int32)
        if tri.size % 3 or not np.array_equal(tri, np.asarray(idx).reshape(-1)):
            raise ValueError("triangles: [m, 3] indices that fit an int")
        return xyz, tri

    def _mesh_voxels(self, voxels, shell=None):
        """voxels= of the two mesh methods: None leaves FS3D_OPT_MESH_VOXELS as it is, "reference" / "conservative" set it (it stays set).
        shell= likewise for FS3D_OPT_MESH_SHELL: "box" / "cross"."""
        if voxels is not None:
            if voxels not in MESH_VOXELS:
                raise ValueError("voxels is 'reference' or 'conservative'")
            self.set_option(OPT_MESH_VOXELS, MESH_VOXELS[voxels])
        if shell is not None:
            if shell not in MESH_SHELL:
                raise ValueError("shell is 'box' or 'cross'")
            self.set_option(OPT_MESH_SHELL, MESH_SHELL[shell])

    @staticmethod
    def _mesh_velocities(w, nvert):
        """wx, wy, wz (float32) of vertex velocities w [n, 3]"""
        w = np.asarray(w, np.float32).reshape(-1, 3)
        if len(w) != nvert:
            raise ValueError("one velocity per vertex")
        return [np.ascontiguousarray(w[:, a]) for a in range(3)]

    def _mesh_args(self, g, w, idx, baseT, wallT):
        """The mesh (g, idx) as the C ABI takes it; unless w is None, with its vertex velocities and wallT (the _vel entries)."""
        xyz, tri = self._mesh_arrays(g, idx)
        wv, wt = ([], []) if w is None else (self._mesh_velocities(w, len(xyz[0])), [float(wallT)])
        return [_p(a) for a in xyz + wv] + [len(xyz[0]), _p(tri), tri.size // 3, float(baseT)] + wt

    def _voxelize_dev(self, fn, what, g, w, idx, baseT, wallT, arrays, voxels, shell=None):
        self._mesh_voxels(voxels, shell)
        ptrs = self._dev_ptrs(what, arrays)
        self._chk(fn(self.h, *self._mesh_args(g, w, idx, baseT, wallT), *ptrs))

    def _update_shape3d(self, fn, g, w, idx, baseT, wallT, voxels, shell=None):
        self._mesh_voxels(voxels, shell)
        return self._update(fn, *self._mesh_args(g, w, idx, baseT, wallT))

    def voxelize_shape3d_dev(self, g, idx, baseT, type, bc_vel, bc_temp, vx, vy, vz, T, voxels=None, shell=None):
        """Grid3D::Build + FloodFill + the Node array on the device: the mesh (g, idx) of shape3d.Shape3D.subframe(t) voxelised into
        seven arrays on the context's device -- torch tensors or raw pointers, as update_nodes_dev takes them.  The context's
        geometry is not touched.  voxels= / shell= of every mesh method: None leaves FS3D_OPT_MESH_VOXELS / FS3D_OPT_MESH_SHELL as
        they are, a word of MESH_VOXELS / MESH_SHELL sets the option, and it stays set ("cross", the thin shell, needs "conservative")."""
        self._voxelize_dev(self.lib.fs3d_voxelize_shape3d_dev, "voxelize_shape3d_dev", g, None, idx, baseT, None, [type, bc_vel, bc_temp, vx, vy, vz, T], voxels, shell)

    def update_nodes_shape3d(self, g, idx, baseT, voxels=None, shell=None):
        """update_nodes with the voxelisation of the mesh (g, idx) as the source: 12 bytes per vertex travel, the node arrays are
        written by kernels.  Same contract as update_nodes."""
        return self._update_shape3d(self.lib.fs3d_update_nodes_shape3d, g, None, idx, baseT, None, voxels, shell)

    def voxelize_shape3d_vel_dev(self, g, w, idx, baseT, wallT, type, bc_vel, bc_temp, vx, vy, vz, T, voxels=None, shell=None):
        """voxelize_shape3d_dev with walls that carry the velocity of the mesh -- w [n, 3], what shape3d.Shape3D.subframe_velocity(t)
        returns -- and the temperature wallT (conservative voxelisation only)."""
        self._voxelize_dev(self.lib.fs3d_voxelize_shape3d_vel_dev, "voxelize_shape3d_vel_dev", g, w, idx, baseT, wallT,
                           [type, bc_vel, bc_temp, vx, vy, vz, T], voxels, shell)

    def update_nodes_shape3d_vel(self, g, w, idx, baseT, wallT, voxels=None, shell=None):
        """update_nodes_shape3d with walls that carry the velocity of the mesh (w [n, 3]) and the temperature wallT (conservative
        voxelisation only).  Same contract as update_nodes."""
        return self._update_shape3d(self.lib.fs3d_update_nodes_shape3d_vel, g, w, idx, baseT, wallT, voxels, shell)

    def update_nodes_shape3d_slab(self, g, idx, baseT, voxels=None, shell=None):
        """update_nodes_shape3d on an x-slab (or a whole-grid context): the vertices g are in GLOBAL grid coordinates, every rank of a
        group is given the same mesh and voxelises and fills the global grid on its own device; no rank waits for another."""
        return self._update_shape3d(self.lib.fs3d_update_nodes_shape3d_slab, g, None, idx, baseT, None, voxels, shell)

    def update_nodes_shape3d_vel_slab(self, g, w, idx, baseT, wallT, voxels=None, shell=None):
        """update_nodes_shape3d_vel on an x-slab (or a whole-grid context), as update_nodes_shape3d_slab."""
        return self._update_shape3d(self.lib.fs3d_update_nodes_shape3d_vel_slab, g, w, idx, baseT, wallT, voxels, shell)

    def flood_fill_global_dev(self, type):
        """flood_fill_dev on a device array of the GLOBAL grid's node types, from any context (an x-slab too): the fill the two
        mesh entries of a slab run."""
        self._chk(self.lib.fs3d_flood_fill_global_dev(self.h, self._dev_ptrs("flood_fill_global_dev", [type])[0]))

    def flood_fill_dev(self, type):
        """FloodFill alone on a device array of node types (uint8 torch tensor or raw pointer) of the context's dims, in place."""
        self._chk(self.lib.fs3d_flood_fill_dev(self.h, self._dev_ptrs("flood_fill_dev", [type])[0]))

    def mesh_fill_rounds(self):
        """Rounds of directional passes the last flood fill on this context ran (the closing one without a change included)."""
        n = C.c_int(0)
        self._chk(self.lib.fs3d_mesh_fill_rounds(self.h, C.byref(n)))
        return n.value

    def clear_outer_cells(self, layer, baseT):
        """Solver3D::ClearOutterCells on one layer: U, V, W := 0 and T := baseT on the NODE_OUT cells."""
        self._chk(self.lib.fs3d_clear_outer_cells(self.h, layer, float(baseT)))

    def fill_fresh_cells(self, layer, max_rounds=0):
        """fs3d_fill_fresh_cells: the cells of `layer` that the last update_nodes* turned NODE_IN take the mean of their fluid
        neighbours (fresh_cells.fill_fresh_cells is the rule), from the snapshot OPT_FRESH_CELLS keeps.
        Returns (fresh, filled, rounds, left).  On a slab of a group with OPT_FRESH_CELLS_SLABS: a collective call, every rank makes
        it with the same arguments; fresh, filled and left count the slab's own cells, rounds is the group's."""
        info = (C.c_longlong * 4)()
        self._chk(self.lib.fs3d_fill_fresh_cells(self.h, layer, max_rounds, info))
        return tuple(info)

    def fill_fresh_cells_dev(self, prev_type, layer, max_rounds=0):
        """The stateless form: prev_type is the node types before the update, on the context's device -- a uint8 torch tensor
        (contiguous, of the grid's size) or a raw device pointer (int), as update_nodes_dev takes its arrays.  On a slab of a group
        (the collective form): the types of the slab's own planes, as a raw device pointer."""
        info = (C.c_longlong * 4)()
        self._chk(self.lib.fs3d_fill_fresh_cells_dev(self.h, self._dev_ptrs("fill_fresh_cells_dev", [prev_type])[0], layer, max_rounds, info))
        return tuple(info)

    def last_fill_device_ms(self):
        """Device time of the last fill_fresh_cells* call (measured while enable_timing is on, else 0)."""
        ms = C.c_float(0)
        self._chk(self.lib.fs3d_last_fill_device_ms(self.h, C.byref(ms)))
        return ms.value

    def last_update_device_ms(self):
        """Device time of the last update_nodes* call (measured while enable_timing is on, else 0)."""
        ms = C.c_float(0)
        self._chk(self.lib.fs3d_last_update_device_ms(self.h, C.byref(ms)))
        return ms.value

    GEOMETRY_INFO = ("segments_x", "segments_y", "segments_z", "bound_cells", "stale_in_cells", "dead_lines_x", "dead_lines_y",
                     "dead_lines_z", "uniform_groups_x", "uniform_groups_y", "shared_columns_x", "shared_columns_y", "code_digest",
                     "device_allocs_and_frees")

    def dead_lines(self, d):
        """The dead-line bytes of direction d of the context's planes (uint8, X: [dimy, dimz], Y: [dimx, dimz], Z: [dimx, dimy]);
        test and measurement aid."""
        n = C.c_longlong(0)
        self._chk(self.lib.fs3d_geometry_dead_lines(self.h, d, None, C.byref(n)))
        out = np.empty(n.value, np.uint8)
        self._chk(self.lib.fs3d_geometry_dead_lines(self.h, d, _p(out), None))
        nx, ny, nz = self.dims
        return out.reshape([(ny, nz), (nx, nz), (nx, ny)][d])

    def geometry_info(self):
        """fs3d_geometry_info as a dict (keys: Solver.GEOMETRY_INFO); measurement and test aid."""
        info = (C.c_longlong * len(self.GEOMETRY_INFO))()
        self._chk(self.lib.fs3d_geometry_info(self.h, info))
        return dict(zip(self.GEOMETRY_INFO, list(info)))

    # -- reference-shaped interface -----------------------------------------------
    def UpdateBoundaries(self):
        self._chk(self.lib.fs3d_update_boundaries(self.h))

    def TimeStep(self, dt, num_global, num_local, computeError=True):
        """Returns diffError.  Raises Fs3dError(status ERR_DIVERGED) where the reference throws."""
        err = C.c_double(0.0)
        self._chk(self.lib.fs3d_time_step(self.h, dt, num_global, num_local, int(computeError), C.byref(err)))
        return err.value

    def time_step_async(self, dt, num_global, num_local):
        self._chk(self.lib.fs3d_time_step_async(self.h, dt, num_global, num_local))

    def synchronize(self):
        self._chk(self.lib.fs3d_synchronize(self.h))

    def GetLayer(self, outdims=(0, 0, 0)):
        od = [o or d for o, d in zip(outdims, self.dims)]
        outV = np.empty(od + [3], dtype=self.dtype)
        outT = np.empty(od, dtype=np.float64)
        self._chk(self.lib.fs3d_get_layer(self.h, _p(outV), _p(outT), *outdims))
        return outV, outT

    def GetLayerRows(self, outV, outT, outdims=(0, 0, 0)):
        """This slab's rows of the GLOBAL result: outV [odx, ody, odz, 3] (the context's precision) and outT [odx, ody, odz]
        (float64) are the arrays of the whole output grid, shared by the slabs of a group (0 = the global dim); the rows i whose
        source plane i*gx/odx this context owns are written.  Returns them as (i0, i1) -- slab.out_rows."""
        od = tuple(o or d for o, d in zip(outdims, self.gdims))
        for a, shape, dt in ((outV, od + (3,), self.dtype), (outT, od, np.float64)):
            if not isinstance(a, np.ndarray) or a.shape != shape or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("GetLayerRows: C-contiguous arrays of the whole output grid, outV in the context's precision, outT float64")
        rows = (C.c_int * 2)()
        self._chk(self.lib.fs3d_get_layer_rows(self.h, _p(outV), _p(outT), *outdims, rows))
        return rows[0], rows[1]

    def GetLayerDev(self, outV, outT, outdims=(0, 0, 0)):
        """The same with the two arrays on the context's device -- torch tensors (contiguous, of the whole output grid's size; the
        context's precision and float64) or raw device pointers (int).  Returns (i0, i1) after the enqueue: read after synchronize()."""
        n = int(np.prod([o or d for o, d in zip(outdims, self.gdims)]))

        def ptr(a, size, numel):
            if isinstance(a, int):
                return C.c_void_p(a)
            if not a.is_cuda or not a.is_contiguous() or a.element_size() != size or a.numel() != numel:
                raise ValueError("GetLayerDev: contiguous device tensors of the whole output grid, outV in the context's precision, outT float64")
            return C.c_void_p(a.data_ptr())
        rows = (C.c_int * 2)()
        self._chk(self.lib.fs3d_get_layer_dev(self.h, ptr(outV, self.dtype.itemsize, 3 * n), ptr(outT, 8, n), *outdims, rows))
        return rows[0], rows[1]

    GET_LAYER_INFO = ("samples", "bytes_to_host", "device_allocs")

    def get_layer_info(self):
        """fs3d_get_layer_info as a dict (keys: Solver.GET_LAYER_INFO): what the last GetLayer* call wrote and copied, and the
        device allocations of all of them; measurement and test aid."""
        info = (C.c_longlong * len(self.GET_LAYER_INFO))()
        self._chk(self.lib.fs3d_get_layer_info(self.h, info))
        return dict(zip(self.GET_LAYER_INFO, list(info)))

    # -- kernel-level access ------------------------------------------------------
    def sweep(self, d, dt, l_cur, l_temp, l_next, merge=False):
        self._chk(self.lib.fs3d_sweep(self.h, d, dt, l_cur, l_temp, l_next, int(merge)))

    def merge(self, l_src, l_dest):
        self._chk(self.lib.fs3d_merge(self.h, l_src, l_dest))

    def eval_div_error(self, layer=LAYER_NEXT):
        err, cnt = C.c_double(0.0), C.c_longlong(0)
        self._chk(self.lib.fs3d_eval_div_error(self.h, layer, C.byref(err), C.byref(cnt)))
        return err.value, cnt.value

    def download_layer(self, layer):
        out = [np.empty(self.dims, dtype=self.dtype) for _ in range(4)]
        self._chk(self.lib.fs3d_download_layer(self.h, layer, *[_p(a) for a in out]))
        return out

    def upload_layer(self, layer, fields):
        arrs = [None if f is None else np.ascontiguousarray(f, self.dtype) for f in fields]
        for a in arrs:
            assert a is None or a.shape == tuple(self.dims)
        self._chk(self.lib.fs3d_upload_layer(self.h, layer, *[_p(a) for a in arrs]))

    def profile_sweep(self, d, dt, l_cur=LAYER_CUR, l_temp=LAYER_TEMP, l_next=LAYER_NEXT, max_blocks=4096):
        """[blocks, 8 waves, 8 stamps] shader-clock stamps of one pipelined sweep (measurement aid)."""
        buf = np.zeros((max_blocks, 8, 8), dtype=np.uint64)   # up to 8 waves per workgroup (unused waves stay 0)
        nb = C.c_int(0)
        self._chk(self.lib.fs3d_profile_sweep(self.h, d, dt, l_cur, l_temp, l_next,
                                              buf.ctypes.data_as(C.POINTER(C.c_ulonglong)), max_blocks, C.byref(nb)))
        return buf[:nb.value]

    def last_sweep_kernels(self):
        """{"X": "part", "Y": "part", "Z": "pipe"}: what the last sweep of each direction really ran."""
        out = {}
        for d, nm in enumerate("XYZ"):
            k, sg = C.c_int(0), C.c_int(0)
            self._chk(self.lib.fs3d_last_sweep_kernel(self.h, d, C.byref(k), C.byref(sg)))
            out[nm] = KERNEL_NAMES.get(k.value, str(k.value)) + ("-segmented" if sg.value & 1 else "") + \
                {0: "", 1: "+pipelined-ranks", 2: "+reduced-interface", 3: "+reduced-interface(on-chip)"}[(sg.value >> 1) & 3] + \
                ("+all-to-all" if sg.value & 8 else "")
        return out

    LAUNCH_FIELDS = {0: ("family",), 1: ("family", "M", "NCH", "LT", "XB", "order", "workgroups"),
                     2: ("family", "LPL", "NW", "LG", "n_grp", "workgroups")}

    def last_sweep_launch(self, d, pass_=0):
        """The partition kernel instance and launch of the last sweep of direction d: {"family": 1, "M": 16, "NCH": 16, "LT": 32,
        "XB": 0, "order": 0x440, "workgroups": 2048}, {"family": 2, "LPL": 64, "NW": 1, "LG": 16, "n_grp": 16, "workgroups": 1024},
        or {"family": 0} where that pass (1: the interface pass of a reduced-interface X sweep) launched no partition kernel."""
        out = (C.c_int * 8)()
        self._chk(self.lib.fs3d_last_sweep_launch(self.h, d, pass_, out))
        return dict(zip(self.LAUNCH_FIELDS[out[0]], out))

    def profiler_events(self):
        """{event name of the reference's Profiler: (total ms, count)} since enable_timing(True)"""
        names, ms, n = (C.c_char_p * N_EVENTS)(), (C.c_float * N_EVENTS)(), (C.c_int * N_EVENTS)()
        self._chk(self.lib.fs3d_profiler_events(self.h, names, ms, n))
        return {names[k].decode(): (ms[k], n[k]) for k in range(N_EVENTS)}

    def enable_timing(self, on=True):
        self._chk(self.lib.fs3d_enable_timing(self.h, int(on)))

    def last_step_timing(self):
        ms, n = (C.c_float * 4)(), (C.c_int * 4)()
        self._chk(self.lib.fs3d_last_step_timing(self.h, ms, n))
        return list(ms), list(n)


class LocalGroup:
    """In-process slab group (fs3d_local_group_create): one Solver per slab, each driven by its own
    thread.  `run(fn)` calls fn(rank, solver) on every slab concurrently and returns the results."""

    def __init__(self, nodes, params, nranks, dtype=np.float32, devices=None):
        from .slab import slab_range
        self.lib = load()
        self.h = C.c_void_p()
        st = self.lib.fs3d_local_group_create(nranks, C.byref(self.h))
        if st != OK:
            raise Fs3dError(st, "fs3d_local_group_create")
        self.solvers = []
        for r in range(nranks):
            s = Solver(nodes, params, dtype=dtype, device=(devices[r] if devices else 0),
                       x_range=slab_range(nodes.dimx, r, nranks))
            s.comm_init_local(self, r)
            self.solvers.append(s)

    def run(self, fn):
        import threading
        out, exc = [None] * len(self.solvers), [None] * len(self.solvers)

        def work(r):
            try:
                out[r] = fn(r, self.solvers[r])
            except BaseException as e:      # noqa: BLE001 - re-raised below
                exc[r] = e
                try:
                    self.solvers[r].comm_abort()        # the other slab threads return ERR_COMM instead of waiting for ever
                except Exception:
                    pass
        th = [threading.Thread(target=work, args=(r,)) for r in range(len(self.solvers))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in exc:
            if e is not None:
                raise e
        return out

    def close(self):
        for s in self.solvers:
            s.close()
        self.solvers = []
        if self.h:
            self.lib.fs3d_local_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shape2d_bottom(dimx, dimy, dz, depth, depth_var):
    """The per-column `bottom` table of the extrusion as the library computes it (host only, no GPU): int32 [dimx, dimy]."""
    out = np.empty((dimx, dimy), np.int32)
    st = load().fs3d_shape2d_bottom(dimx, dimy, float(dz), float(depth), float(depth_var), out.ctypes.data_as(C.POINTER(C.c_int)))
    if st != OK:
        raise Fs3dError(st, "fs3d_shape2d_bottom: bad dims, or depth / dz gives no active_dimz")
    return out


def fluid_params(dtype, Re, Pr, lam):
    """FluidParams(Re, Pr, lambda), Geometry.h:545-552, rounded to FTYPE."""
    dt = np.dtype(dtype).type
    return (dt(1.0), dt(1.0 / Re), dt(1.0 / (Re * Pr)), dt((lam - 1) / (lam * Re)))


def fluid_params_physical(dtype, vis, rho, R, k, cv):
    """FluidParams(vis, rho, R, k, cv), Geometry.h:554-561."""
    dt = np.dtype(dtype).type
    return (dt(R), dt(vis / rho), dt(k / (rho * cv)), dt(vis / (rho * cv)))
