// The conservative voxelisation of a Shape3D mesh, its thin shell and the velocity its walls carry: the one C++ statement of the
// rule, shared by the kernels (k_geom_voxel_mesh, k_geom_mesh_nodes_vel of kernels_geom.hip) and the host loader (host/Shape3D.h).
// The specification, with the slack's derivation and why the thin shell separates, is the numpy twin cmc_fluid_solver_amd/shape3d.py
// (_voxel_setup, _voxel_triangle, wall_weights, wall_velocity): fp32 vertices, every float64 operation the twin's, in its order,
// rounded after each one.
// No HIP header: any C++17 compiler will do (tests/voxel_rule_test.cpp runs it on a CPU).
// REQUIREMENT: every translation unit that includes this file is compiled with -ffp-contract=off and without -ffast-math.  The
// expressions below are plain; a fused multiply-add rounds once where the rule rounds twice, and that moves a wall.
#pragma once
#include <math.h>

#ifdef __FAST_MATH__
#error "fs3d_voxel.h: compile without -ffast-math (and with -ffp-contract=off): the rule rounds after every operation"
#endif

#ifdef __HIPCC__
#define FS3D_VOXEL_FN __host__ __device__ __forceinline__
#define FS3D_VOXEL_UNROLL _Pragma("unroll")
#else
#define FS3D_VOXEL_FN inline
#define FS3D_VOXEL_UNROLL
#endif

constexpr double VOXEL_SLACK = 5.8207660913467407e-11;        // 2^-34
constexpr double VOXEL_DEGENERATE = 5.9604644775390625e-08;   // 2^-24: the squared normal below which a triangle has no plane
constexpr float VOXEL_COORD_MAX = 4096.0f;                    // the largest magnitude of a vertex coordinate, in grid cells

struct VoxelEdge { double wa, wb, c; };

FS3D_VOXEL_FN double voxel_val(const VoxelEdge &e, double x, double y) { return (e.wa * x + e.wb * y) + e.c; }
FS3D_VOXEL_FN bool voxel_pass(const VoxelEdge &e, double x, double y) { return voxel_val(e, x, y) >= 0.0; }
// the thin shell: the centre of the unit square of a projection lies inside all three edges -- each value reaches its half-width
FS3D_VOXEL_FN bool voxel_centre(const VoxelEdge (&e)[3], const double (&hw)[3], double x, double y)
{
    return voxel_val(e[0], x, y) >= hw[0] && voxel_val(e[1], x, y) >= hw[1] && voxel_val(e[2], x, y) >= hw[2];
}
// component c of (x, y, z) by selection: an index that is not a constant would put the set-up into scratch on the device
template <typename T> FS3D_VOXEL_FN T voxel_sel(int c, T x, T y, T z) { return c == 0 ? x : (c == 1 ? y : z); }

// One triangle against the grid.  The three axes are renamed (a, b, d), cyclic so that orientation is kept, with d the depth axis:
// the normal's dominant axis, for a degenerate triangle (no plane) the axis of its smallest extent.
struct VoxelSetup {
    int o[3];                   // the first cell of the clipped bounding box, in x, y, z
    int cnt[3];                 // cells of the box along a, b, d
    int a, b, d;
    bool degenerate;
    VoxelEdge edge[3][3];       // projections (a, b), (b, d), (d, a): the three edge functions of each, in box-local coordinates
    double na, nb, nd;          // the normal, renamed (zero for a degenerate triangle)
    double c1, c2;              // the plane: s + c1 >= 0 and s + c2 <= 0 for s = na ia + nb ib + nd k
    // THIN only: per projection k of third axis C, the half-widths of its three edge values and of the plane value, and n_C != 0
    double hw[3][3], hn[3];
    bool along[3];
};

// The set-up of the triangle p[vertex][x, y, z] on a grid of dimx x dimy x dimz cells; false: no cell of the grid meets its box.
template <bool THIN>
FS3D_VOXEL_FN bool voxel_setup(const float (&p)[3][3], int dimx, int dimy, int dimz, VoxelSetup &s)
{
    const int dims[3] = {dimx, dimy, dimz};
    int n[3];
    FS3D_VOXEL_UNROLL
    for (int c = 0; c < 3; c++) {
        const float mn = fminf(p[0][c], fminf(p[1][c], p[2][c])), mx = fmaxf(p[0][c], fmaxf(p[1][c], p[2][c]));
        const int l = (int)ceilf(mn) - 1, h = (int)floorf(mx);                 // cells i with i + 1 >= mn and i <= mx
        const int lo = l > 0 ? l : 0, hi = h < dims[c] - 1 ? h : dims[c] - 1;
        if (lo > hi) return false;
        s.o[c] = lo; n[c] = hi - lo + 1;
    }
    // float64 from here on: the local vertices and the edges are exact
    double q[3][3], amax = 0.0;
    FS3D_VOXEL_UNROLL
    for (int i = 0; i < 3; i++)
        FS3D_VOXEL_UNROLL
        for (int c = 0; c < 3; c++) { q[i][c] = (double)p[i][c] - (double)s.o[c]; amax = fmax(amax, fabs(q[i][c])); }
    const double S = (amax + 2.0) * VOXEL_SLACK;
    const double e0x = q[1][0] - q[0][0], e0y = q[1][1] - q[0][1], e0z = q[1][2] - q[0][2];
    const double e1x = -(q[0][0] - q[2][0]), e1y = -(q[0][1] - q[2][1]), e1z = -(q[0][2] - q[2][2]);
    double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const double nn = (nx * nx + ny * ny) + nz * nz;
    const bool degenerate = !(nn >= VOXEL_DEGENERATE);
    int d = 0;
    if (degenerate) {
        double ext[3];
        FS3D_VOXEL_UNROLL
        for (int c = 0; c < 3; c++) ext[c] = fmax(q[0][c], fmax(q[1][c], q[2][c])) - fmin(q[0][c], fmin(q[1][c], q[2][c]));
        nx = 0.0; ny = 0.0; nz = 0.0;
        double best = ext[0];
        if (ext[1] < best) { d = 1; best = ext[1]; }
        if (ext[2] < best) d = 2;
    } else {
        double best = fabs(nx);
        if (fabs(ny) > best) { d = 1; best = fabs(ny); }
        if (fabs(nz) > best) d = 2;
    }
    const int a = d == 2 ? 0 : d + 1, b = d == 0 ? 2 : d - 1;
    double t[3][3];                                         // the vertices renamed: index 0, 1, 2 = a, b, d
    FS3D_VOXEL_UNROLL
    for (int i = 0; i < 3; i++) { t[i][0] = voxel_sel(a, q[i][0], q[i][1], q[i][2]); t[i][1] = voxel_sel(b, q[i][0], q[i][1], q[i][2]); t[i][2] = voxel_sel(d, q[i][0], q[i][1], q[i][2]); }
    const double nr[3] = {voxel_sel(a, nx, ny, nz), voxel_sel(b, nx, ny, nz), voxel_sel(d, nx, ny, nz)};
    s.cnt[0] = voxel_sel(a, n[0], n[1], n[2]); s.cnt[1] = voxel_sel(b, n[0], n[1], n[2]); s.cnt[2] = voxel_sel(d, n[0], n[1], n[2]);
    s.a = a; s.b = b; s.d = d; s.degenerate = degenerate;
    FS3D_VOXEL_UNROLL
    for (int k = 0; k < 3; k++) {                           // projections (a, b), (b, d), (d, a)
        const int A = k, B = (k + 1) % 3, C = (k + 2) % 3;
        FS3D_VOXEL_UNROLL
        for (int j = 0; j < 3; j++) {
            const int v0 = j, v1 = (j + 1) % 3;
            const double eA = t[v1][A] - t[v0][A], eB = t[v1][B] - t[v0][B];
            const double wa = nr[C] >= 0.0 ? -eB : eB, wb = nr[C] >= 0.0 ? eA : -eA;              // the inward normal of the edge
            double tmin = wa * t[0][A] + wb * t[0][B];
            tmin = fmin(tmin, wa * t[1][A] + wb * t[1][B]);
            tmin = fmin(tmin, wa * t[2][A] + wb * t[2][B]);
            const double cmax = fmax(wa, 0.0) + fmax(wb, 0.0);
            const double sl = S * (fabs(wa) + fabs(wb));
            s.edge[k][j].wa = wa; s.edge[k][j].wb = wb; s.edge[k][j].c = (cmax - tmin) + sl;
        }
    }
    const double na = nr[0], nb = nr[1], nd = nr[2];
    double c1 = 0.0, c2 = 0.0;
    if (!degenerate) {
        const double t0 = (na * t[0][0] + nb * t[0][1]) + nd * t[0][2], t1 = (na * t[1][0] + nb * t[1][1]) + nd * t[1][2],
                     t2 = (na * t[2][0] + nb * t[2][1]) + nd * t[2][2];
        const double tmin = fmin(t0, fmin(t1, t2)), tmax = fmax(t0, fmax(t1, t2));
        const double cmax = (fmax(na, 0.0) + fmax(nb, 0.0)) + fmax(nd, 0.0), cmin = (fmin(na, 0.0) + fmin(nb, 0.0)) + fmin(nd, 0.0);
        const double sl = S * ((fabs(na) + fabs(nb)) + fabs(nd));
        c1 = (cmax - tmin) + sl; c2 = (cmin - tmax) - sl;
    }
    s.na = na; s.nb = nb; s.nd = nd; s.c1 = c1; s.c2 = c2;
    if constexpr (THIN) {
        FS3D_VOXEL_UNROLL
        for (int k = 0; k < 3; k++) {
            FS3D_VOXEL_UNROLL
            for (int j = 0; j < 3; j++) s.hw[k][j] = 0.5 * (fabs(s.edge[k][j].wa) + fabs(s.edge[k][j].wb));
            s.hn[k] = 0.5 * (fabs(nr[k]) + fabs(nr[(k + 1) % 3]));
            s.along[k] = nr[(k + 2) % 3] != 0.0;
        }
    }
    return true;
}

// One column (ia, ib) of the (a, b) projection, in box-local cells.
struct VoxelColumn {
    double pa, pb, g;           // g = na ia + nb ib
    int k0, k1;                 // the depth range to walk: it only bounds the loop, every cell in it runs all remaining tests
    bool centre_d;              // THIN only: the column's centre line (along d) passes inside the three edges
};

// false: the column fails an edge test of its projection.  A column takes its depth range from the plane, one cell of margin each
// way; a degenerate triangle has no plane and walks the box's depth.
template <bool THIN>
FS3D_VOXEL_FN bool voxel_column(const VoxelSetup &s, int ia, int ib, VoxelColumn &c)
{
    const double pa = (double)ia, pb = (double)ib;
    if (!voxel_pass(s.edge[0][0], pa, pb) || !voxel_pass(s.edge[0][1], pa, pb) || !voxel_pass(s.edge[0][2], pa, pb)) return false;
    int k0 = 0, k1 = s.cnt[2] - 1;
    double g = 0.0;
    if (!s.degenerate) {                                    // s + c1 >= 0 and s + c2 <= 0 for s = g + nd k
        g = s.na * pa + s.nb * pb;
        const double lo = (-s.c1 - g) / s.nd, hi = (-s.c2 - g) / s.nd, lim = 1048576.0;
        const int f = (int)floor(fmin(fmax(fmin(lo, hi), -lim), lim)) - 1, l = (int)ceil(fmin(fmax(fmax(lo, hi), -lim), lim)) + 1;
        k0 = f > 0 ? f : 0;
        k1 = l < s.cnt[2] - 1 ? l : s.cnt[2] - 1;
    }
    c.pa = pa; c.pb = pb; c.g = g; c.k0 = k0; c.k1 = k1;
    if constexpr (THIN) c.centre_d = s.along[0] && voxel_centre(s.edge[0], s.hw[0], pa, pb);
    return true;
}

// The cell k of the column: the six remaining edge tests, the plane, and with THIN the filter -- of the cells that pass, a
// non-degenerate triangle sets those whose centre cross (the three unit segments through the centre, one along each axis) it
// meets: inside the edges of the segment's projection, and in depth.
template <bool THIN>
FS3D_VOXEL_FN bool voxel_cell(const VoxelSetup &s, const VoxelColumn &c, int k)
{
    const double pa = c.pa, pb = c.pb, pd = (double)k;
    if (!voxel_pass(s.edge[1][0], pb, pd) || !voxel_pass(s.edge[1][1], pb, pd) || !voxel_pass(s.edge[1][2], pb, pd)) return false;
    if (!voxel_pass(s.edge[2][0], pd, pa) || !voxel_pass(s.edge[2][1], pd, pa) || !voxel_pass(s.edge[2][2], pd, pa)) return false;
    if (!s.degenerate) {
        const double v = c.g + s.nd * pd;
        if (!(v + s.c1 >= 0.0) || !(v + s.c2 <= 0.0)) return false;
        if constexpr (THIN) {
            const double u1 = v + s.c1, u2 = v + s.c2;
            if (!(c.centre_d && u1 >= s.hn[0] && u2 <= -s.hn[0]) &&
                !(s.along[1] && u1 >= s.hn[1] && u2 <= -s.hn[1] && voxel_centre(s.edge[1], s.hw[1], pb, pd)) &&
                !(s.along[2] && u1 >= s.hn[2] && u2 <= -s.hn[2] && voxel_centre(s.edge[2], s.hw[2], pd, pa))) return false;
        }
    }
    return true;
}

// ---- walls that carry the mesh's velocity ------------------------------------------------------------------------------------------
// The velocity of the triangle (q0, q1, q2) -- local to the cell's corner, q_i = (double)v_i - (i, j, k) -- with vertex velocities
// W0, W1, W2 at the cell's centre c = (1/2, 1/2, 1/2): float64, to be rounded once.  e0 = q1 - q0, e1 = q2 - q0, r = c - q0,
// n = e0 x e1, nn = (nx nx + ny ny) + nz nz.  nn >= VOXEL_DEGENERATE: b1 = ((r x e1) . n) / nn, b2 = ((e0 x r) . n) / nn,
// b0 = (1 - b1) - b2 (the barycentric coordinates of the centre's orthogonal projection onto the plane), m_i = max(b_i, 0),
// w_i = m_i / ((m0 + m1) + m2).  Else the longest of the edges (0,1), (1,2), (2,0) by squared length, the first of equals: t = the
// parameter of the centre's projection onto it clamped to [0, 1] (0 for a zero length), 1 - t and t on its ends, 0 on the third
// vertex.  The result is (w0 W0 + w1 W1) + w2 W2 per component.
struct D3 { double x, y, z; };
FS3D_VOXEL_FN D3 d3_sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
FS3D_VOXEL_FN D3 d3_cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
FS3D_VOXEL_FN double d3_dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

FS3D_VOXEL_FN D3 wall_velocity(D3 q0, D3 q1, D3 q2, D3 W0, D3 W1, D3 W2)
{
    const D3 c = {0.5, 0.5, 0.5};
    const D3 e0 = d3_sub(q1, q0), e1 = d3_sub(q2, q0), r = d3_sub(c, q0);
    const D3 n = d3_cross(e0, e1);
    const double nn = d3_dot(n, n);
    double w0, w1, w2;
    if (nn >= VOXEL_DEGENERATE) {
        const double b1 = d3_dot(d3_cross(r, e1), n) / nn, b2 = d3_dot(d3_cross(e0, r), n) / nn, b0 = (1.0 - b1) - b2;
        const double m0 = fmax(b0, 0.0), m1 = fmax(b1, 0.0), m2 = fmax(b2, 0.0);
        const double s = (m0 + m1) + m2;
        w0 = m0 / s; w1 = m1 / s; w2 = m2 / s;
    } else {                                               // the longest edge, the first of equals
        const D3 d0 = e0, d1 = d3_sub(q2, q1), d2 = d3_sub(q0, q2);
        const double l0 = d3_dot(d0, d0), l1 = d3_dot(d1, d1), l2 = d3_dot(d2, d2);
        int best = 0;
        double l = l0;
        if (l1 > l) { best = 1; l = l1; }
        if (l2 > l) { best = 2; l = l2; }
        const D3 a = best == 0 ? q0 : (best == 1 ? q1 : q2), d = best == 0 ? d0 : (best == 1 ? d1 : d2);
        double t = 0.0;
        if (l > 0.0) t = fmin(fmax(d3_dot(d3_sub(c, a), d) / l, 0.0), 1.0);
        const double u = 1.0 - t;                          // on the edge's first end, t on its second, 0 on the third vertex
        w0 = best == 0 ? u : (best == 2 ? t : 0.0);
        w1 = best == 1 ? u : (best == 0 ? t : 0.0);
        w2 = best == 2 ? u : (best == 1 ? t : 0.0);
    }
    return {(w0 * W0.x + w1 * W1.x) + w2 * W2.x, (w0 * W0.y + w1 * W1.y) + w2 * W2.y, (w0 * W0.z + w1 * W1.z) + w2 * W2.z};
}
