"""Shape3D input surface: the reference's `in_fmt Shape3D` triangle-mesh geometry rasterised into the Node array.

Python twin of cmc_fluid_solver_amd/host/Shape3D.h (same operations in np.float32 where the reference computes in FTYPE = float;
the header lists the reference lines and the two deliberate deviations: NODE_BOUND cells read as zero-filled memory --
BC_NOSLIP, v = 0, T = 0 -- and cells addressed outside the grid are ignored; a third one concerns a moving run: nodes_of() is a
function of the current grid alone, where the reference's repeated Prepare_CPU keeps T = 0 on cells that once were walls).  Restates
  Grid3D::Load3DShape / Init / Prepare3D_Shape / ComputeSubframeInfo / Build / RasterPolygon / ProjectPointOnPolygon /
  RasterLine / FloodFill                         (FluidSolver3D/Grid3D.cpp:351-431, 676-946)
  BBox3D::Build                                  (Common/Geometry.h:510-529)
Wall velocities (conservative voxelisation only; the reference reads a velocity per vertex and drops it in RasterPolygon): see
wall_weights below -- every NODE_BOUND cell takes the velocity of its owner triangle at the projection of the cell's centre.
Pinned to the reference (r3): tests/test_ref_golden.py holds this loader cell for cell to the node arrays of the reference's own
Grid3D on the shipped box_pipe_3D and tetra meshes and on a two-frame icosphere at five times (tests/golden/ref_*_3D_*.npz,
ref_tetra_f32.npz); tests/test_shape3d.py compares the C++ loader with this twin.
"""
import math

import numpy as np

from .grids import BC_NOSLIP, NODE_BOUND, NODE_IN, NODE_OUT, Nodes
from .shape2d import align_by_32

F = np.float32
GRID_SCALE_FACTOR = F(0.001)
COMP_EPS = 1e-8
BBOX_PADDING = 0.02
INF = 1e10


def parse_shape3d(text):
    """Grid3D::Load3DShape (Grid3D.cpp:373-416): frames of (vertices [n,3] float32, velocities [n,3], triangles [m,3] int)."""
    tok = text.replace("\r", "").split()
    it = iter(tok)
    num = lambda: F(float(next(it).replace(",", ".")))
    frames = []
    for _ in range(int(next(it))):
        nv = int(next(it))
        v = np.zeros((nv, 3), np.float32); w = np.zeros((nv, 3), np.float32)
        for k in range(nv):
            v[k] = [F(num() * GRID_SCALE_FACTOR) for _ in range(3)]
            w[k] = [num() for _ in range(3)]
        nt = int(next(it))
        idx = np.array([int(next(it)) for _ in range(3 * nt)], np.int64).reshape(nt, 3)
        if idx.size and (idx.min() < 0 or idx.max() >= nv):
            raise ValueError("Shape3D: triangle index outside the vertex list")
        frames.append({"v": v, "vel": w, "idx": idx, "duration": 1.0 / 75})
    return frames


# ---- conservative voxelisation (voxels="conservative"): the specification; its one C++ statement, constants included, is -----------
# csrc/fs3d_voxel.h, which host/Shape3D.h and csrc/kernels_geom.hip both run
# A cell becomes NODE_BOUND iff a triangle overlaps its closed unit box [i, i+1] x [j, j+1] x [k, k+1]: separating axes in the
# Schwarz-Seidel form.  The bounding box is compared in grid coordinates, where nothing is rounded (floor / ceil of the fp32
# vertices): its slack is zero.  Every other inequality is  f(p) = w.p + c >= 0  for an axis w (an edge normal of a projection, or
# the plane's normal), c = (max of w over the unit box) - (min of w.q_i over the three vertices) + S |w|_1, on coordinates local to
# the integer corner `o` of the triangle's clipped bounding box; S |w|_1 is the slack: the unit box grown by S.
# Comparing the box's interval along w with the triangle's *interval* is a valid separating-axis test for any w whatever, so the
# rounding of w (cancellation in the normal of a thin triangle) can never drop a cell: only the evaluation of f has to be guarded.
# Arithmetic: the vertices are fp32, everything computed from them is float64, in a fixed order, uncontracted, so that numpy, g++
# and the kernel produce the same bits.  In float64 the local vertices q = v - o (fp32 minus an integer below 2^13) and the edge
# vectors are exact, so a vertex shared by two triangles is the same point seen from both origins; the cell coordinates p are
# exact; the normal is the cross product of exact edges, good to 2^-52 of its terms.
# Why not fp32: at coordinates near 100 one fp32 rounding is 6e-6 of a cell -- in the evaluation, and through the normal's
# rounding in the width of the triangle's interval along it -- and a face that misses a cell corner by 1e-6 (the shipped tetra
# mesh has 172 such corners) could not be told from one that touches it.
# Where the slack comes from.  u = 2^-53, L = max |q| + 2 (a local cell corner p + 1 is at most max q + 1), every |w_c x_c| <= |w_c| L.
# Roundings of one inequality in units of u L |w|_1: w.q_i -- products <= 1, sums <= 2; cmax - tmin <= 1; adding the slack <= 1;
# w.p -- products exact, sums <= 2; the last sum <= 1: at most 8, second-order terms and the roundings of cmax and of S |w|_1 (a few
# u |w|_1, without the factor L >= 2) fit into 4 more: the rounding bound is 12 u L |w|_1 = 1.3e-15 L |w|_1.  The slack is set far
# above it, S = VOXEL_SLACK * L = 2^-34 L (6e-9 of a cell at L = 100, below 5e-7 whatever the mesh: coordinates are at most
# VOXEL_COORD_MAX in magnitude, so L <= 2^13 + 3), so that a float64 restatement with a noise of its own (tests/watertight_cases.py)
# can hold the result to it.  So: a cell whose box overlaps the triangle is always set, and a set cell's box grown by
# VOXEL_TOL * L = (2^-34 + 12 u) L overlaps it.
VOXEL_SLACK = 2.0 ** -34
VOXEL_TOL = 2.0 ** -34 + 12 * 2.0 ** -53
VOXEL_COORD_MAX = 4096.0
# A triangle whose squared normal is below this is degenerate -- two or three equal vertices,
# collinear ones, or an area below 2^-13 of a cell's face: it is within 2^-6 of a cell of its longest edge.  It has no plane to take
# a depth range from; its three edges are tested as segments in the three projections (for collinear vertices the two shorter ones
# lie on the longest: the cells of the longest edge, no more), never its bounding box.
VOXEL_DEGENERATE = 2.0 ** -24
_VOXEL_AXES = ((1, 2, 0), (2, 0, 1), (0, 1, 2))      # (a, b, d): the column plane and the depth axis, cyclic, by depth axis d
_VOXEL_EDGES = ((0, 1), (1, 2), (2, 0))
VOXEL_MODES = ("reference", "conservative")
# ---- thin shell (voxels="conservative", shell="cross"): a filter inside the conservative test -------------------------------------
# The flood fill spreads over the 6-neighbourhood, so a shell only has to be 6-separating: where a triangle cuts the straight
# line between two neighbouring cell centres, one of the two cells has to be a wall.  That line is one half of the centre cross of
# each of the two cells -- the three unit segments through a cell's centre, one parallel to each axis -- so it is enough to set the
# cells whose centre cross the triangle meets, not every cell whose box it touches.
# Rule.  A non-degenerate triangle sets a cell of its clipped box iff the conservative test holds (every v[k][j] >= 0, s + c1 >= 0,
# s + c2 <= 0, with v[k][j] = (wA x + wB y) + c the nine edge values and s = (na pa + nb pb) + nd pd the plane value of
# _voxel_triangle) and some projection k = 0, 1, 2 = (a, b), (b, d), (d, a), of third axis C = d, a, b, has all of
#   n_C != 0,   v[k][j] >= (|wA| + |wB|) / 2 for j = 0, 1, 2,   s + c1 >= H_k,   s + c2 <= -H_k,   H_k = (|n_A| + |n_B|) / 2.
# Why this is the centre segment along C.  In projection k that segment is a point, the centre of the unit square: c holds the
# maximum of w over the square, which exceeds w at the centre by (|wA| + |wB|) / 2, so comparing v with that half-width instead of
# 0 tests the point where the conservative test tests the square.  Along the normal the box's interval is wider than the
# segment's by (|n|_1 - |n_C|) / 2 = H_k on each side.  n_C = 0 is a triangle parallel to the segment: an edge-on contact, which the
# other two projections see.  The slack S and the rounding bound are the conservative test's own (the half-widths are exact
# halves of sums it already forms), so a centre segment that truly meets the triangle always sets its cell, and the thin shell is
# a subset of the conservative one by construction.
# Degenerate triangles (nn < VOXEL_DEGENERATE) keep the conservative treatment: a needle below the area threshold can still be cut
# by a centre line, and a superset there is harmless.  The owner of a wall cell is the smallest index of the triangles whose
# *thin* test sets it.
SHELL_MODES = ("box", "cross")
WALL_VELOCITY_SOURCES = ("motion", "file")
NO_OWNER = -1


# ---- wall velocities of a mesh (conservative voxelisation only): the specification of wall_velocity in csrc/fs3d_voxel.h, ----
# which host/Shape3D.h and k_geom_mesh_nodes_vel share
# Owner.  The owner of a NODE_BOUND cell is the triangle of smallest index whose test sets the cell (the mask of
# _voxel_triangle: the conservative test, with shell="cross" the thin one): a minimum over a set, so it does not depend on the
# order in which triangles are visited.  Where several triangles overlap a cell the choice is arbitrary; the velocity field of a mesh is continuous across shared vertices, so another
# choice moves the value by the velocity gradient times a cell.
# Weights.  float64 from the fp32 vertices, every operation rounded once, in the order written here, uncontracted.  Coordinates
# are local to the cell's own corner, q_i = (double)v_i - (i, j, k) (exact for |v| <= VOXEL_COORD_MAX), the centre is c = (1/2, 1/2, 1/2).
#   e0 = q1 - q0, e1 = q2 - q0, r = c - q0, n = e0 x e1, nn = (nx nx + ny ny) + nz nz
#   nn >= VOXEL_DEGENERATE: b1 = ((r x e1) . n) / nn, b2 = ((e0 x r) . n) / nn, b0 = (1 - b1) - b2 -- the barycentric coordinates of
#     the centre's orthogonal projection onto the plane; m_i = max(b_i, 0); w_i = m_i / ((m0 + m1) + m2)
#   else: the longest of the edges (0,1), (1,2), (2,0) by squared length (the first wins ties), t = the parameter of the centre's
#     projection onto it clamped to [0, 1] (0 for an edge of zero length): 1 - t and t on its two ends, 0 on the third vertex
# a cross product is (ay bz - az by, az bx - ax bz, ax by - ay bx), a dot product (x x' + y y') + z z'.
# Velocity.  Per component (w0 W0 + w1 W1) + w2 W2 from the fp32 vertex velocities W_i, rounded once to the solver's real type.

def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def wall_weights(p, cell):
    """The three weights (float64) of the triangle p [3][3] (fp32 vertices in grid coordinates) at the cells `cell` = (i, j, k):
    scalars or equal-shaped integer arrays.  Every operation is a float64 numpy operation, elementwise: rounded once, never fused."""
    D = np.float64
    ijk = [np.asarray(c, D) for c in cell]
    q = [[np.asarray(p[i][c], D) - ijk[c] for c in range(3)] for i in range(3)]
    e0 = [q[1][c] - q[0][c] for c in range(3)]; e1 = [q[2][c] - q[0][c] for c in range(3)]
    r = [D(0.5) - q[0][c] for c in range(3)]
    n = _cross(e0, e1)
    nn = _dot(n, n)
    with np.errstate(all="ignore"):
        b1 = _dot(_cross(r, e1), n) / nn
        b2 = _dot(_cross(e0, r), n) / nn
        b0 = (D(1.0) - b1) - b2
        m = [np.maximum(b, D(0.0)) for b in (b0, b1, b2)]
        s = (m[0] + m[1]) + m[2]
        plane = [x / s for x in m]
        # degenerate: the longest edge, the first of equals
        d = [[q[j][c] - q[i][c] for c in range(3)] for i, j in _VOXEL_EDGES]
        l = [_dot(x, x) for x in d]
        rr = [[D(0.5) - q[i][c] for c in range(3)] for i, _ in _VOXEL_EDGES]
        t = [np.where(l[k] > 0, np.minimum(np.maximum(_dot(rr[k], d[k]) / l[k], D(0.0)), D(1.0)), D(0.0)) for k in range(3)]
    best = np.where(l[1] > l[0], 1, 0)
    best = np.where(l[2] > np.where(best == 1, l[1], l[0]), 2, best)
    zero = np.zeros_like(nn)
    edge = []
    for v in range(3):                                   # vertex v: 1 - t as the first end of edge v, t as the second end of edge v - 1
        prev = (v + 2) % 3
        edge.append(np.where(best == v, D(1.0) - t[v], np.where(best == prev, t[prev], zero)))
    deg = ~(nn >= VOXEL_DEGENERATE)
    return [np.where(deg, edge[v], plane[v]) for v in range(3)]


def wall_velocity(w, W):
    """(w0 W0 + w1 W1) + w2 W2 per component, float64, from the weights of wall_weights and the fp32 vertex velocities W [3][3]."""
    D = np.float64
    return [(w[0] * np.asarray(W[0][c], D) + w[1] * np.asarray(W[1][c], D)) + w[2] * np.asarray(W[2][c], D) for c in range(3)]


class Shape3D:
    shell = "box"                                         # (a class default: twins made without __init__ keep the conservative shell)

    def __init__(self, frames, dx, dy, dz, align, time=0.0, voxels="reference", wall_velocity=None, shell="box"):
        if voxels not in VOXEL_MODES:
            raise ValueError("Shape3D: voxels is 'reference' or 'conservative'")
        if shell not in SHELL_MODES:
            raise ValueError("Shape3D: shell is 'box' or 'cross'")
        if shell == "cross" and voxels != "conservative":
            raise ValueError("Shape3D: shell='cross' needs voxels='conservative' (the thin shell is a filter inside its overlap test)")
        self.shell = shell
        if wall_velocity is not None and wall_velocity not in WALL_VELOCITY_SOURCES:
            raise ValueError("Shape3D: wall_velocity is None, 'motion' or 'file'")
        if wall_velocity is not None and voxels != "conservative":
            raise ValueError("Shape3D: wall velocities need voxels='conservative' (the owner of a wall cell is defined by its overlap test)")
        self.voxels = voxels
        self.wall_velocity = wall_velocity                # prepare(t) then keeps owner and wall_v (build with the velocities of time t)
        self.frames = frames
        self.dx, self.dy, self.dz = dx, dy, dz
        allv = np.concatenate([fr["v"] for fr in frames], axis=0)
        mn = np.minimum(allv.min(axis=0), F(INF)).astype(np.float32); mx = np.maximum(allv.max(axis=0), F(-INF)).astype(np.float32)
        w = (mx - mn).astype(np.float32)
        pad = (w * F(BBOX_PADDING)).astype(np.float32)
        mn = (mn - pad).astype(np.float32); mx = (mx + pad).astype(np.float32)
        self.bbox = tuple(mn) + tuple(mx)
        dims = [int(math.ceil(float(F(mx[a] - mn[a])) / d)) + 1 for a, d in enumerate((dx, dy, dz))]
        if align:
            dims = [align_by_32(d) for d in dims]
        self.dimx, self.dimy, self.dimz = dims
        h = np.array([F(dx), F(dy), F(dz)], np.float32)
        for fr in frames:
            fr["g"] = ((fr["v"] - mn).astype(np.float32) / h).astype(np.float32)
        self.prepare(time)

    def _locate(self, time):
        """ComputeSubframeInfo (Grid3D.cpp:905-946): (frame, the next frame -- wrapped --, s as float32)"""
        nf = len(self.frames)
        a = [0.0]
        for fr in self.frames:
            a.append(a[-1] + fr["duration"])
        r = math.fmod(time, a[-1])
        frame = 0
        for i in range(1, nf):
            if a[i] < r:
                frame = i
        return frame, (frame + 1) % nf, F((r - a[frame]) / (a[frame + 1] - a[frame]))

    def subframe(self, time):
        """ComputeSubframeInfo + the interpolation of Prepare3D_Shape (Grid3D.cpp:905-946): (vertices in grid coordinates
        [n, 3] float32, triangles [m, 3]) of the mesh at `time` -- what build() and the device voxeliser take."""
        frame, nxt, s = self._locate(time)
        i_s = F(F(1) - s)
        f0, f1 = self.frames[frame], self.frames[nxt]
        g = ((f0["g"] * i_s).astype(np.float32) + (f1["g"] * s).astype(np.float32)).astype(np.float32)
        return g, f0["idx"]

    def subframe_velocity(self, time, source="motion"):
        """The vertex velocities [n, 3] float32 of the mesh at `time`, in the solver's velocity units, beside subframe(time).
        "motion": (P[f+1] - P[f]) (1 / Duration[f]) on the physical vertices, fp32 in the order of shape2d.py's border velocities;
        f is subframe's frame and f + 1 wraps as there.  The vertices move linearly over a frame interval, so the velocity is
        constant over it; a one-frame mesh is at rest.
        "file": the file's velocity columns as the reference interpolates them (Grid3D.cpp:915), W[f] (1 - s) + W[f+1] s, taken
        as they are (their unit is not documented)."""
        if source not in WALL_VELOCITY_SOURCES:
            raise ValueError("Shape3D: a velocity source is 'motion' or 'file'")
        frame, nxt, s = self._locate(time)
        f0, f1 = self.frames[frame], self.frames[nxt]
        if source == "motion":
            m = F(1.0 / f0["duration"])
            return ((f1["v"] - f0["v"]).astype(np.float32) * m).astype(np.float32)
        i_s = F(F(1) - s)
        return ((f0["vel"] * i_s).astype(np.float32) + (f1["vel"] * s).astype(np.float32)).astype(np.float32)

    def prepare(self, time):
        g, idx = self.subframe(time)
        self.build(g, idx, None if self.wall_velocity is None else self.subframe_velocity(time, self.wall_velocity))

    # ---- rasteriser -----------------------------------------------------------------------------------------------
    def _set(self, i, j, k, c):
        if 0 <= i < self.dimx and 0 <= j < self.dimy and 0 <= k < self.dimz:
            self.type[i, j, k] = c

    @staticmethod
    def _horizon(p1, p2, p):
        if abs(float(F(p1[1] - p2[1]))) < COMP_EPS:
            return (p[0], p[1])
        return (F(p1[0] + F(F(F(p2[0] - p1[0]) * F(p[1] - p1[1])) / F(p2[1] - p1[1]))), p[1])

    def _project(self, d_, i, j, tp, n, d):
        o = [(1, 2), (0, 2), (0, 1)][d_]
        with np.errstate(all="ignore"):
            kf = F(F(F(-d) - F(F(tp[0] * n[o[0]]) + F(tp[1] * n[o[1]]))) / n[d_])
        if not np.isfinite(kf) or abs(float(kf)) > 2e9:
            return
        k = int(kf)
        lim = (self.dimx, self.dimy, self.dimz)[d_]
        if 0 <= k < lim:
            if d_ == 0:
                self._set(k, i, j, NODE_BOUND)
            elif d_ == 1:
                self._set(i, k, j, NODE_BOUND)
            else:
                self._set(i, j, k, NODE_BOUND)

    def _scan_half(self, p, yend, dp, e1, e2, di, d_, n, d):
        bound = 4 * (self.dimx + self.dimy + self.dimz) + 16
        while p[1] < yend:
            j = int(p[1])
            last_i = int(self._horizon(e1, e2, p)[0])
            i, guard = int(p[0]), 0
            while i != last_i + di:
                guard += 1
                if guard > bound:
                    raise ValueError("Shape3D: a scan line of a polygon never reaches its end cell (the reference loops there)")
                self._project(d_, i, j, (F(i), p[1]), n, d)
                i += di
            p = (F(p[0] + dp[0]), F(p[1] + dp[1]))
        return p

    def _raster_polygon(self, p1, p2, p3):
        eq = lambda a, b: all(abs(float(F(a[q] - b[q]))) < COMP_EPS for q in range(3))
        if eq(p1, p2) and eq(p1, p3):
            return
        a = [F(p2[q] - p1[q]) for q in range(3)]; b = [F(p3[q] - p1[q]) for q in range(3)]
        n = [F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))]
        ln = F(np.sqrt(F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))))
        if not ln > 0:
            return
        t = F(F(1) / ln)
        n = [F(c * t) for c in n]
        d = F(-F(F(F(p1[0] * n[0]) + F(p1[1] * n[1])) + F(p1[2] * n[2])))
        maxv = max(abs(n[0]), abs(n[1]), abs(n[2]))
        d_ = 0
        for q in range(3):
            if abs(float(F(maxv - abs(n[q])))) < COMP_EPS:
                d_ = q
        o = [(1, 2), (0, 2), (0, 1)][d_]
        pp = [(p[o[0]], p[o[1]]) for p in (p1, p2, p3)]
        if pp[2][1] < pp[1][1]: pp[1], pp[2] = pp[2], pp[1]
        if pp[0][1] > pp[1][1]: pp[0], pp[1] = pp[1], pp[0]
        if pp[2][1] < pp[1][1]: pp[1], pp[2] = pp[2], pp[1]
        pp1, pp2, pp3 = pp
        mid = self._horizon(pp1, pp3, pp2)
        dir1 = (F(mid[0] - pp1[0]), F(mid[1] - pp1[1])); dir2 = (F(pp3[0] - mid[0]), F(pp3[1] - mid[1]))
        steps1 = int(max(abs(dir1[0]), abs(dir1[1]))) + 1; steps2 = int(max(abs(dir2[0]), abs(dir2[1]))) + 1
        dp1 = (F(dir1[0] / F(steps1)), F(dir1[1] / F(steps1))); dp2 = (F(dir2[0] / F(steps2)), F(dir2[1] / F(steps2)))
        di = 1 if mid[0] < pp2[0] else -1
        p = self._scan_half(pp1, mid[1], dp1, pp1, pp2, di, d_, n, d)
        self._scan_half(p, pp3[1], dp2, pp2, pp3, di, d_, n, d)

    def _raster_line(self, p1, p2):
        dr = [F(p2[q] - p1[q]) for q in range(3)]
        steps = int(max(abs(dr[0]), abs(dr[1]), abs(dr[2]))) + 1
        dp = [F(c / F(steps)) for c in dr]
        p = list(p1)
        for _ in range(steps + 1):
            self._set(int(p[0]), int(p[1]), int(p[2]), NODE_BOUND)
            p = [F(p[q] + dp[q]) for q in range(3)]

    # ---- conservative voxeliser ---------------------------------------------------------------------------------------
    def _voxel_setup(self, p):
        """The set-up (voxel_setup of csrc/fs3d_voxel.h: wave-uniform in k_geom_voxel_mesh) for the triangle p[3][3] (fp32): None when its bounding box misses the grid,
        else (o, n, axes, edge functions [projection][edge] = (wA, wB, c), plane (na, nb, nd, c1, c2) or None), all float64."""
        dims = (self.dimx, self.dimy, self.dimz)
        o, n = [], []
        for c in range(3):
            mn, mx = min(p[0][c], p[1][c], p[2][c]), max(p[0][c], p[1][c], p[2][c])
            lo, hi = max(int(math.ceil(mn)) - 1, 0), min(int(math.floor(mx)), dims[c] - 1)      # cells i with i + 1 >= mn and i <= mx
            if lo > hi:
                return None
            o.append(lo); n.append(hi - lo + 1)
        # float64 from here on (Python floats), every operation rounded once: the local vertices and the edge vectors are exact
        q = [[float(p[i][c]) - float(o[c]) for c in range(3)] for i in range(3)]
        S = (max(abs(q[i][c]) for i in range(3) for c in range(3)) + 2.0) * VOXEL_SLACK
        e = [[q[j][c] - q[i][c] for c in range(3)] for i, j in _VOXEL_EDGES]
        e0, e1 = e[0], [-x for x in e[2]]                                                      # v1 - v0, v2 - v0
        nrm = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
        nn = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]
        degenerate = not nn >= VOXEL_DEGENERATE
        if degenerate:                                   # depth along the axis of the smallest extent: few cells per column
            ext = [max(q[0][c], q[1][c], q[2][c]) - min(q[0][c], q[1][c], q[2][c]) for c in range(3)]
            nrm = [0.0, 0.0, 0.0]
            d = 0
            if ext[1] < ext[0]: d = 1
            if ext[2] < ext[d]: d = 2
        else:                                            # depth along the normal's dominant axis
            d = 0
            if abs(nrm[1]) > abs(nrm[0]): d = 1
            if abs(nrm[2]) > abs(nrm[d]): d = 2
        axes = _VOXEL_AXES[d]
        edges = []
        for k in range(3):                               # projections (a, b), (b, d), (d, a): (A, B) cyclic, C the third axis
            A, B, C = axes[k], axes[(k + 1) % 3], axes[(k + 2) % 3]
            fns = []
            for j in range(3):
                eA, eB = e[j][A], e[j][B]
                wA, wB = (-eB, eA) if nrm[C] >= 0 else (eB, -eA)                               # the inward normal of the edge
                tmin = min(wA * q[v][A] + wB * q[v][B] for v in range(3))
                cmax = max(wA, 0.0) + max(wB, 0.0)
                fns.append((wA, wB, (cmax - tmin) + S * (abs(wA) + abs(wB))))
            edges.append(fns)
        plane = None
        if not degenerate:
            a, b = axes[0], axes[1]
            na, nb, nd = nrm[a], nrm[b], nrm[d]
            t = [(na * q[v][a] + nb * q[v][b]) + nd * q[v][d] for v in range(3)]
            cmax = (max(na, 0.0) + max(nb, 0.0)) + max(nd, 0.0); cmin = (min(na, 0.0) + min(nb, 0.0)) + min(nd, 0.0)
            sl = S * ((abs(na) + abs(nb)) + abs(nd))
            plane = (na, nb, nd, (cmax - min(t)) + sl, (cmin - max(t)) - sl)
        return o, n, axes, edges, plane

    def _voxel_triangle(self, p, t=0):
        st = self._voxel_setup(p)
        if st is None:
            return
        o, n, (a, b, d), edges, plane = st
        pa = np.arange(n[a], dtype=np.float64)[:, None, None]; pb = np.arange(n[b], dtype=np.float64)[None, :, None]
        pd = np.arange(n[d], dtype=np.float64)[None, None, :]
        ev = lambda fn, x, y: ((fn[0] * x + fn[1] * y) + fn[2]) >= 0          # float64 arrays: rounded after every operation
        col = ev(edges[0][0], pa, pb) & ev(edges[0][1], pa, pb) & ev(edges[0][2], pa, pb)
        k0, k1 = np.zeros(col.shape, np.int64), np.full(col.shape, n[d] - 1, np.int64)
        if plane is not None:
            na, nb, nd, c1, c2 = plane
            g = na * pa + nb * pb
            lo, hi = (-c1 - g) / nd, (-c2 - g) / nd                             # s + c1 >= 0 and s + c2 <= 0 for s = g + nd k
            lim = 2.0 ** 20
            k0 = np.maximum(np.floor(np.clip(np.minimum(lo, hi), -lim, lim)).astype(np.int64) - 1, 0)      # one cell of margin each way:
            k1 = np.minimum(np.ceil(np.clip(np.maximum(lo, hi), -lim, lim)).astype(np.int64) + 1, n[d] - 1)  # the range only bounds the loop
        kk = np.arange(n[d])[None, None, :]
        m = col & (kk >= k0) & (kk <= k1)
        for fn in edges[1]:
            m = m & ev(fn, pb, pd)
        for fn in edges[2]:
            m = m & ev(fn, pd, pa)
        if plane is not None:
            s = g + nd * pd
            m = m & ((s + c1) >= 0) & ((s + c2) <= 0)
            if self.shell == "cross":                     # the centre cross: some projection sees the cell's centre inside, in depth too
                val = lambda fn, x, y: (fn[0] * x + fn[1] * y) + fn[2]
                xy = ((pa, pb), (pb, pd), (pd, pa))
                nr = (na, nb, nd)
                thin = np.zeros(m.shape, bool)
                for k in range(3):
                    if nr[(k + 2) % 3] == 0:
                        continue
                    H = 0.5 * (abs(nr[k]) + abs(nr[(k + 1) % 3]))
                    hit = ((s + c1) >= H) & ((s + c2) <= -H)
                    for fn in edges[k]:
                        hit = hit & (val(fn, *xy[k]) >= 0.5 * (abs(fn[0]) + abs(fn[1])))
                    thin = thin | hit
                m = m & thin
        m = np.transpose(m, [(a, b, d).index(c) for c in range(3)])
        box = (slice(o[0], o[0] + n[0]), slice(o[1], o[1] + n[1]), slice(o[2], o[2] + n[2]))
        self.type[box][m] = NODE_BOUND
        own = self.owner[box]                             # the smallest index of the triangles that set the cell
        own[m & ((own == NO_OWNER) | (own > t))] = t

    def _wall_velocities(self, g, idx, vel):
        """wall_v = (vx, vy, vz) float64 [dimx, dimy, dimz]: wall_velocity(wall_weights(owner)) on NODE_BOUND cells, 0 elsewhere"""
        out = [np.zeros(self.type.shape, np.float64) for _ in range(3)]
        ci, cj, ck = np.nonzero(self.owner != NO_OWNER)
        if len(ci):
            tri = np.asarray(idx).reshape(-1, 3)[self.owner[ci, cj, ck]]          # [cells, 3]
            p = [[np.asarray(g, np.float32)[tri[:, v], c] for c in range(3)] for v in range(3)]
            W = [[np.asarray(vel, np.float32)[tri[:, v], c] for c in range(3)] for v in range(3)]
            for c, u in enumerate(wall_velocity(wall_weights(p, (ci, cj, ck)), W)):
                out[c][ci, cj, ck] = u
        return tuple(out)

    def build(self, g, idx, vel=None):
        """The grid of the mesh (g, idx); with vertex velocities vel [n, 3] (conservative voxelisation only) also wall_v.
        The conservative voxelisation always keeps `owner` (int, NO_OWNER off the walls)."""
        self.type = np.full((self.dimx, self.dimy, self.dimz), NODE_IN, np.uint8)
        self.owner, self.wall_v = None, None
        if vel is not None and self.voxels != "conservative":
            raise ValueError("Shape3D: wall velocities need the conservative voxelisation")
        if self.voxels == "conservative":
            g = np.asarray(g, np.float32)
            if len(g) and not (np.abs(g) <= VOXEL_COORD_MAX).all():
                raise ValueError("Shape3D: a vertex coordinate is not finite or exceeds 4096 grid cells in magnitude (conservative voxelisation)")
            self.owner = np.full(self.type.shape, NO_OWNER, np.int64)
        if vel is not None:
            vel = np.asarray(vel, np.float32)
            if vel.shape != np.asarray(g).shape or not np.isfinite(vel).all():
                raise ValueError("Shape3D: one finite velocity per vertex")
        for t, (i1, i2, i3) in enumerate(idx):
            p1, p2, p3 = (tuple(F(c) for c in g[q]) for q in (i1, i2, i3))
            if self.voxels == "conservative":
                self._voxel_triangle((p1, p2, p3), t)
                continue
            self._raster_polygon(p1, p2, p3)
            self._raster_line(p1, p2); self._raster_line(p1, p3); self._raster_line(p3, p2)
        # flood fill NODE_OUT from (0,0,0) through NODE_IN cells, 6-neighbourhood (scipy labels the same set)
        from scipy import ndimage
        free = self.type == NODE_IN
        free[0, 0, 0] = True
        lab, _ = ndimage.label(free)
        self.type[lab == lab[0, 0, 0]] = NODE_OUT
        if vel is not None:
            self.wall_v = self._wall_velocities(g, idx, vel)


def load_shape3d(path_or_text, dx, dy, dz, baseT=1.0, align=True, is_text=False, voxels="reference", wall_velocity=None, wall_T=0.0, time=0.0,
                 shell="box"):
    """Grid3D(dx,dy,dz,baseT) + LoadFromFile + Prepare_CPU(time) for a Shape3D input -> (Nodes, Shape3D).  wall_velocity ("motion" /
    "file", conservative voxelisation only) and wall_T: what the walls carry, see nodes_of; shell ("box" / "cross", the latter with the
    conservative voxelisation only): the thin shell."""
    text = path_or_text if is_text else open(path_or_text, "r").read()
    sh = Shape3D(parse_shape3d(text), dx, dy, dz, align, time, voxels=voxels, wall_velocity=wall_velocity, shell=shell)
    return nodes_of(sh, dx, dy, dz, baseT, sh.wall_v, wall_T), sh


def nodes_of(sh, dx, dy, dz, baseT=1.0, wall_v=None, wall_T=0.0):
    """The Node array of a prepared Shape3D grid: NODE_BOUND cells carry NOSLIP, v = 0, T = 0 (what the reference's run holds
    there: tests/golden/ref_box_pipe_3D_f32.npz), every other cell T = baseT.  With wall_v = (vx, vy, vz) (sh.wall_v of a grid
    built with vertex velocities) the NODE_BOUND cells carry those, float64 here and rounded once by whoever narrows them to the
    solver's real type; wall_T is their temperature (through a float, like baseT)."""
    shape = sh.type.shape
    z8 = np.zeros(shape, np.uint8)
    zero = np.zeros(shape, np.float64)
    T = np.where(sh.type == NODE_BOUND, float(F(wall_T)), float(F(baseT)))
    v = [zero, zero.copy(), zero.copy()] if wall_v is None else [np.where(sh.type == NODE_BOUND, a, 0.0) for a in wall_v]
    return Nodes(sh.dimx, sh.dimy, sh.dimz, dx, dy, dz, sh.type.copy(), z8 + BC_NOSLIP, z8 + BC_NOSLIP, v[0], v[1], v[2], T)


def write_mesh(path, frames):
    """A Shape3D file from [(vertices in mm [n,3], triangles [m,3])]: the test inputs are written with this."""
    with open(path, "w") as f:
        f.write("%d\n" % len(frames))
        for v, tri in frames:
            f.write("%d\n" % len(v))
            for p in v:
                f.write("%.6g %.6g %.6g 0 0 0\n" % tuple(p))
            f.write("%d\n" % len(tri))
            for t in tri:
                f.write("%d %d %d\n" % tuple(t))
