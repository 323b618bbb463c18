// Shape3D input surface in C++: the reference's `in_fmt Shape3D` triangle-mesh geometry rasterised into the Node array
// the solver consumes.  Operation for operation (FTYPE = float, the reference's geometry type):
//   Grid3D::Load3DShape                         (FluidSolver3D/Grid3D.cpp:373-431)
//   BBox3D::Build, Grid3D::Init                 (Common/Geometry.h:510-529, Grid3D.cpp:351-371)
//   Grid3D::Prepare3D_Shape / ComputeSubframeInfo / Build / RasterPolygon / ProjectPointOnPolygon / RasterLine / FloodFill
//                                               (Grid3D.cpp:676-946)
// File: frames; per frame: vertices, per vertex "x y z  vx vy vz", triangles, 3 indices each.  Frame duration 1/75 s; the
// cycle length of a Shape3D run is Config::frame_time and GetFrame is always 0 (Grid3D.cpp:303-336).
// Shape3D::voxels = 1 replaces the rasteriser (not the fill) by a conservative voxelisation, which the reference does not have: see
// VoxelTriangle below, the rule in csrc/fs3d_voxel.h (shared with the kernels) and its derivation in cmc_fluid_solver_amd/shape3d.py.  Shape3D::shell = 1 keeps of that shell the cells whose centre
// cross a triangle meets (the thin, 6-separating shell: the same file).
// Shape3D::wall_velocity (conservative voxelisation only) gives the NODE_BOUND cells the velocity of the mesh, which the reference
// reads per vertex, interpolates (Grid3D.cpp:915) and then drops in RasterPolygon / RasterLine: see WallVelocity below.
// Deviations, on purpose (a third one, of the moving loop, stands at FillShape3DNodes below):
//   * NODE_BOUND cells: the reference sets only their type; bc_vel / bc_temp keep whatever `new Node[]` left there
//     (Grid3D.cpp:351-371, 818-838: SetData runs for NODE_IN / NODE_OUT only).  Here they read as zero-filled memory:
//     BC_NOSLIP for both, v = 0, T = 0 (Init's values).
//   * cells addressed outside the grid (the reference writes past its array) are ignored; a scan line that would never reach its
//     end cell (the reference loops until the int wraps) throws.
// Pinned to the reference (r3) through the Python twin cmc_fluid_solver_amd/shape3d.py (same operations; tests/test_shape3d.py compares
// the two cell for cell): the twin equals the node arrays of the reference's own Grid3D on the shipped box_pipe_3D and tetra meshes and
// on a two-frame icosphere at five times (tests/test_ref_golden.py, tests/golden/ref_box_pipe_3D_f32.npz ...); the zero-filled reading
// of the NODE_BOUND cells is what the reference's run holds there.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/fs3d_voxel.h"
#include "AdiSolver3D_hip.h"
#include "Shape2D.h"

namespace fs3d {

struct Shape3DFrame {
    std::vector<float> x, y, z, vx, vy, vz;   // vertices (physical, then grid coordinates) and their velocities (the file's columns; unused by the rasteriser)
    std::vector<float> px, py, pz;            // the physical vertices, kept: the `motion` velocities are their differences
    std::vector<int> idx;                     // 3 per triangle
    double duration = 1.0 / 75;               // Grid3D.cpp:413
};

struct Shape3D {
    static constexpr float GRID_SCALE_FACTOR = 0.001f;       // Grid2D.h:31
    static constexpr double COMP_EPS = 1e-8, BBOX_PADDING = 0.02, INF = 1e10;   // Geometry.h:22-24
    std::vector<Shape3DFrame> frames;
    float bbox[6] = {0, 0, 0, 0, 0, 0};       // pMin.xyz, pMax.xyz
    int dimx = 0, dimy = 0, dimz = 0;
    double dx = 0, dy = 0, dz = 0;
    std::vector<uint8_t> type;
    // 0: the reference's rasteriser (RasterPolygon + RasterLine; not watertight).  1: conservative voxelisation (VoxelTriangle below):
    // NODE_BOUND iff a triangle overlaps the cell's closed unit box, so the shell of a closed mesh is closed for the flood fill.
    // Set it before Load; Prepare(t) honours it.  Same value as FS3D_OPT_MESH_VOXELS.
    int voxels = 0;
    // 0: the conservative shell as it is.  1 (needs voxels = 1): the thin shell -- of the cells a non-degenerate triangle's conservative
    // test sets, those whose centre cross (the three unit segments through the centre, one along each axis) the triangle meets:
    // closed for the fill's 6-neighbourhood, about 0.55 of the cells.  The rule and why it separates stand in
    // cmc_fluid_solver_amd/shape3d.py (SHELL_MODES).  Set it before Load; Prepare(t) honours it.  Same value as FS3D_OPT_MESH_SHELL.
    int shell = 0;
    // What the NODE_BOUND cells carry.  0: v = 0 (the reference's run).  1 (`motion`) / 2 (`file`): the velocity of the mesh at the
    // projection of the cell's centre onto the cell's owner triangle (WallVelocity below), from the vertex velocities
    // SubFrameVelocity gives for that source.  Needs voxels = 1.  Set it before Load; Prepare(t) honours it and keeps `owner` and
    // `cur`, which FillShape3DNodes reads.
    int wall_velocity = 0;
    std::vector<int> owner;                   // per cell: the smallest index of the triangles whose test (with shell = 1: the thin one) sets it, -1 off the walls
    Shape3DFrame cur;                         // the sub-frame of the last Prepare: vertices in grid coordinates, velocities, triangles

    static float num(std::string tok) { std::replace(tok.begin(), tok.end(), ',', '.'); return (float)std::atof(tok.c_str()); }

    void Load(const std::string &path, double dx_, double dy_, double dz_, bool align)
    {
        std::ifstream in(path.c_str());
        if (!in) throw std::runtime_error("cannot open Shape3D file " + path);
        std::vector<std::string> t;
        for (std::string w; in >> w;) t.push_back(w);
        size_t i = 0;
        auto next = [&]() -> const std::string & { if (i >= t.size()) throw std::runtime_error("Shape3D file ends early"); return t[i++]; };
        const int nf = std::atoi(next().c_str());
        if (nf < 1 || (size_t)nf > t.size()) throw std::runtime_error("Shape3D file: bad number of frames");
        frames.assign(nf, Shape3DFrame());
        for (auto &fr : frames) {
            const int nv = std::atoi(next().c_str());
            if (nv < 0 || (size_t)nv > t.size()) throw std::runtime_error("Shape3D file: bad number of vertices");
            for (int k = 0; k < nv; k++) {
                const float px = num(next()), py = num(next()), pz = num(next());
                fr.x.push_back(px * GRID_SCALE_FACTOR); fr.y.push_back(py * GRID_SCALE_FACTOR); fr.z.push_back(pz * GRID_SCALE_FACTOR);
                fr.px.push_back(fr.x.back()); fr.py.push_back(fr.y.back()); fr.pz.push_back(fr.z.back());
                fr.vx.push_back(num(next())); fr.vy.push_back(num(next())); fr.vz.push_back(num(next()));
            }
            const int nt = std::atoi(next().c_str());
            if (nt < 0 || (size_t)nt > t.size()) throw std::runtime_error("Shape3D file: bad number of triangles");
            for (int k = 0; k < 3 * nt; k++) {
                const int v = std::atoi(next().c_str());
                if (v < 0 || v >= nv) throw std::runtime_error("Shape3D: triangle index outside the vertex list");
                fr.idx.push_back(v);
            }
        }
        for (auto &fr : frames)
            if (fr.x.size() != frames[0].x.size()) throw std::runtime_error("Shape3D: frames differ in their number of vertices");
        dx = dx_; dy = dy_; dz = dz_;
        // BBox3D::Build over all frames
        float mn[3] = {(float)INF, (float)INF, (float)INF}, mx[3] = {(float)-INF, (float)-INF, (float)-INF};
        for (auto &fr : frames)
            for (size_t k = 0; k < fr.x.size(); k++) {
                const float p[3] = {fr.x[k], fr.y[k], fr.z[k]};
                for (int a = 0; a < 3; a++) { if (p[a] < mn[a]) mn[a] = p[a]; if (p[a] > mx[a]) mx[a] = p[a]; }
            }
        for (int a = 0; a < 3; a++) {
            const float w = mx[a] - mn[a];
            const float pad = w * (float)BBOX_PADDING;
            mn[a] = mn[a] - pad; mx[a] = mx[a] + pad;
            bbox[a] = mn[a]; bbox[3 + a] = mx[a];
        }
        for (int a = 0; a < 3; a++) {
            const double h = a == 0 ? dx : (a == 1 ? dy : dz);
            if (!(mx[a] >= mn[a]) || !(h > 0) || (double)(mx[a] - mn[a]) / h > 65536.0)
                throw std::runtime_error("Shape3D: the mesh does not give a grid of a sensible size (more than 65536 cells along an axis, or no vertices)");
        }
        // Grid3D::Init
        dimx = (int)std::ceil((float)(mx[0] - mn[0]) / dx) + 1;
        dimy = (int)std::ceil((float)(mx[1] - mn[1]) / dy) + 1;
        dimz = (int)std::ceil((float)(mx[2] - mn[2]) / dz) + 1;
        if (align) { dimx = AlignBy32(dimx); dimy = AlignBy32(dimy); dimz = AlignBy32(dimz); }
        if ((double)dimx * dimy * dimz >= 2147483648.0) throw std::runtime_error("Shape3D: grid of more than 2^31 cells");
        // physical -> grid coordinates (Grid3D.cpp:420-428)
        for (auto &fr : frames)
            for (size_t k = 0; k < fr.x.size(); k++) {
                fr.x[k] = (float)(fr.x[k] - mn[0]) / (float)dx; fr.y[k] = (float)(fr.y[k] - mn[1]) / (float)dy; fr.z[k] = (float)(fr.z[k] - mn[2]) / (float)dz;
            }
        Prepare(0.0);
    }

    int GetFramesNum() const { return (int)frames.size(); }

    // ComputeSubframeInfo(frame, substep) and the interpolation of Grid3D::Prepare3D_Shape(time) (Grid3D.cpp:905-946): the vertices of
    // the mesh at `time`, in grid coordinates; returns the frame whose triangles the sub-frame has.  This is what changes with time:
    // fs3d_update_nodes_shape3d takes these vertices and frames[frame].idx
    size_t SubFrame(double time, std::vector<float> &x, std::vector<float> &y, std::vector<float> &z) const
    {
        float s;
        const size_t frame = Locate(time, s);
        const float is = 1 - s;
        const Shape3DFrame &f0 = frames[frame], &f1 = frames[(frame + 1) % frames.size()];
        const size_t nv = f0.x.size();
        x.resize(nv); y.resize(nv); z.resize(nv);
        for (size_t k = 0; k < nv; k++) {
            x[k] = mix(f0.x[k], is, f1.x[k], s); y[k] = mix(f0.y[k], is, f1.y[k], s); z[k] = mix(f0.z[k], is, f1.z[k], s);
        }
        return frame;
    }

    // The vertex velocities of the mesh at `time`, in the solver's velocity units, beside SubFrame(time); source as wall_velocity.
    // 1 (`motion`): (P[f+1] - P[f]) (1 / Duration[f]) on the physical vertices, fp32 in the order of Shape2D's border velocities;
    //   f is SubFrame's frame and f + 1 wraps as there.  The vertices move linearly over a frame interval, so the velocity is
    //   constant over it; a one-frame mesh is at rest.
    // 2 (`file`): the file's velocity columns as the reference interpolates them (Grid3D.cpp:915), W[f] (1 - s) + W[f+1] s, taken as
    //   they are (their unit is not documented).
    void SubFrameVelocity(double time, int source, std::vector<float> &wx, std::vector<float> &wy, std::vector<float> &wz) const
    {
        if (source != 1 && source != 2) throw std::runtime_error("Shape3D: a velocity source is 1 (motion) or 2 (file)");
        float s;
        const size_t frame = Locate(time, s);
        const float is = 1 - s;
        const Shape3DFrame &f0 = frames[frame], &f1 = frames[(frame + 1) % frames.size()];
        const size_t nv = f0.x.size();
        wx.resize(nv); wy.resize(nv); wz.resize(nv);
        const float m = (float)(1 / (double)f0.duration);
        for (size_t k = 0; k < nv; k++) {
            if (source == 1) { wx[k] = fl(fl(f1.px[k] - f0.px[k]) * m); wy[k] = fl(fl(f1.py[k] - f0.py[k]) * m); wz[k] = fl(fl(f1.pz[k] - f0.pz[k]) * m); }
            else { wx[k] = mix(f0.vx[k], is, f1.vx[k], s); wy[k] = mix(f0.vy[k], is, f1.vy[k], s); wz[k] = mix(f0.vz[k], is, f1.vz[k], s); }
        }
    }

    // Grid3D::Prepare3D_Shape(time): SubFrame + Build (and the velocities of `time` where the walls carry them)
    void Prepare(double time)
    {
        cur.idx = frames[SubFrame(time, cur.x, cur.y, cur.z)].idx;
        if (wall_velocity) SubFrameVelocity(time, wall_velocity, cur.vx, cur.vy, cur.vz);
        Build(cur);
    }

    // ---- wall velocities: wall_velocity of csrc/fs3d_voxel.h (where the rule is stated; the twin: wall_weights / wall_velocity) ----
    // The velocity of triangle t of the sub-frame `cur` at the centre of cell (i, j, k): float64, to be rounded once.
    // The owner of a cell -- the smallest index of the triangles whose conservative test sets it -- is arbitrary where several
    // overlap the cell; the velocity field of a mesh is continuous across shared vertices, so another choice moves the value by
    // the velocity gradient times a cell.
    void WallVelocity(int t, int i, int j, int k, double u[3]) const
    {
        D3 q[3], W[3];
        for (int v = 0; v < 3; v++) {
            const int iv = cur.idx[3 * (size_t)t + v];
            q[v] = {(double)cur.x[iv] - (double)i, (double)cur.y[iv] - (double)j, (double)cur.z[iv] - (double)k};
            W[v] = {(double)cur.vx[iv], (double)cur.vy[iv], (double)cur.vz[iv]};
        }
        const D3 r = ::wall_velocity(q[0], q[1], q[2], W[0], W[1], W[2]);
        u[0] = r.x; u[1] = r.y; u[2] = r.z;
    }

    // Build on a mesh given in grid coordinates (dimx, dimy, dimz set by the caller): what Prepare does with a sub-frame, for
    // callers that bring their own vertices (tests/mesh_voxel_test.cpp)
    void BuildMesh(const Shape3DFrame &fr) { Build(fr); }

private:
    // ComputeSubframeInfo (Grid3D.cpp:905-946): the frame of `time` and the weight s of the one after it
    size_t Locate(double time, float &s) const
    {
        const size_t nf = frames.size();
        std::vector<double> a(nf + 1, 0.0);
        for (size_t i = 1; i <= nf; i++) a[i] = a[i - 1] + frames[i - 1].duration;
        const double r = std::fmod(time, a[nf]);
        size_t frame = 0;
        for (size_t i = 1; i < nf; i++) if (a[i] < r) frame = i;
        s = (float)((r - a[frame]) / (a[frame + 1] - a[frame]));
        return frame;
    }
    static float mix(float a, float wa, float b, float wb) { volatile float x = a * wa, y = b * wb; return x + y; }
    static float fl(float v) { volatile float x = v; return x; }                    // one rounding to float, no contraction
    size_t id(int i, int j, int k) const { return ((size_t)i * dimy + j) * dimz + k; }
    void Set(int i, int j, int k, uint8_t c) { if (i >= 0 && j >= 0 && k >= 0 && i < dimx && j < dimy && k < dimz) type[id(i, j, k)] = c; }

    struct V2 { float x, y; };
    static V2 Horizon(V2 p1, V2 p2, V2 p)              // GetIntersectHorizon (Grid3D.cpp:676-685)
    {
        V2 r; r.y = p.y;
        if (std::fabs(p1.y - p2.y) < COMP_EPS) r.x = p.x;
        else r.x = fl(p1.x + fl(fl(fl(p2.x - p1.x) * fl(r.y - p1.y)) / fl(p2.y - p1.y)));
        return r;
    }
    // ProjectPointOnPolygon (Grid3D.cpp:688-707): back onto the polygon's plane along its dominant axis
    void Project(int dir, int i, int j, V2 tp, const float n[3], float d)
    {
        if (dir == 0) { const int k = (int)(fl(-d - fl(fl(tp.x * n[1]) + fl(tp.y * n[2]))) / n[0]); if (k >= 0 && k < dimx) Set(k, i, j, NODE_BOUND); }
        else if (dir == 1) { const int k = (int)(fl(-d - fl(fl(tp.x * n[0]) + fl(tp.y * n[2]))) / n[1]); if (k >= 0 && k < dimy) Set(i, k, j, NODE_BOUND); }
        else { const int k = (int)(fl(-d - fl(fl(tp.x * n[0]) + fl(tp.y * n[1]))) / n[2]); if (k >= 0 && k < dimz) Set(i, j, k, NODE_BOUND); }
    }
    void ScanHalf(V2 &p, float yend, V2 dp, V2 e1, V2 e2, int di, int dir, const float n[3], float d)
    {
        const long bound = 4l * (dimx + dimy + dimz) + 16;
        for (; p.y < yend;) {
            const int j = (int)p.y;
            const int last_i = (int)Horizon(e1, e2, p).x;
            long guard = 0;
            for (int i = (int)p.x; i != last_i + di; i += di) {
                if (++guard > bound) throw std::runtime_error("Shape3D: a scan line of a polygon never reaches its end cell (the reference loops there)");
                Project(dir, i, j, V2{(float)i, p.y}, n, d);
            }
            p.x = fl(p.x + dp.x); p.y = fl(p.y + dp.y);
        }
    }
    // RasterPolygon (Grid3D.cpp:709-789)
    void RasterPolygon(const float p1[3], const float p2[3], const float p3[3])
    {
        auto eq = [](const float *a, const float *b) { return std::fabs(a[0] - b[0]) < COMP_EPS && std::fabs(a[1] - b[1]) < COMP_EPS && std::fabs(a[2] - b[2]) < COMP_EPS; };
        if (eq(p1, p2) && eq(p1, p3)) return;
        const float a[3] = {fl(p2[0] - p1[0]), fl(p2[1] - p1[1]), fl(p2[2] - p1[2])}, b[3] = {fl(p3[0] - p1[0]), fl(p3[1] - p1[1]), fl(p3[2] - p1[2])};
        float n[3] = {fl(fl(a[1] * b[2]) - fl(a[2] * b[1])), fl(fl(a[2] * b[0]) - fl(a[0] * b[2])), fl(fl(a[0] * b[1]) - fl(a[1] * b[0]))};
        const float len = (float)std::sqrt(fl(fl(fl(n[0] * n[0]) + fl(n[1] * n[1])) + fl(n[2] * n[2])));
        const float t = 1 / len;
        n[0] = fl(n[0] * t); n[1] = fl(n[1] * t); n[2] = fl(n[2] * t);
        const float d = -fl(fl(fl(p1[0] * n[0]) + fl(p1[1] * n[1])) + fl(p1[2] * n[2]));
        const float maxv = std::max(std::fabs(n[0]), std::max(std::fabs(n[1]), std::fabs(n[2])));
        int dir = 0;                                                          // the reference leaves it unset when no test passes (NaN normal)
        if (std::fabs(maxv - std::fabs(n[0])) < COMP_EPS) dir = 0;
        if (std::fabs(maxv - std::fabs(n[1])) < COMP_EPS) dir = 1;
        if (std::fabs(maxv - std::fabs(n[2])) < COMP_EPS) dir = 2;
        if (!(len > 0)) return;                                               // degenerate triangle (collinear vertices): no plane
        V2 pp1, pp2, pp3;
        if (dir == 0) { pp1 = {p1[1], p1[2]}; pp2 = {p2[1], p2[2]}; pp3 = {p3[1], p3[2]}; }
        else if (dir == 1) { pp1 = {p1[0], p1[2]}; pp2 = {p2[0], p2[2]}; pp3 = {p3[0], p3[2]}; }
        else { pp1 = {p1[0], p1[1]}; pp2 = {p2[0], p2[1]}; pp3 = {p3[0], p3[1]}; }
        V2 mid;
        if (pp3.y < pp2.y) { mid = pp3; pp3 = pp2; pp2 = mid; }
        if (pp1.y > pp2.y) { mid = pp1; pp1 = pp2; pp2 = mid; }
        if (pp3.y < pp2.y) { mid = pp3; pp3 = pp2; pp2 = mid; }
        mid = Horizon(pp1, pp3, pp2);
        const V2 dir1{fl(mid.x - pp1.x), fl(mid.y - pp1.y)}, dir2{fl(pp3.x - mid.x), fl(pp3.y - mid.y)};
        const int steps1 = (int)std::max(std::fabs(dir1.x), std::fabs(dir1.y)) + 1, steps2 = (int)std::max(std::fabs(dir2.x), std::fabs(dir2.y)) + 1;
        const V2 dp1{dir1.x / steps1, dir1.y / steps1}, dp2{dir2.x / steps2, dir2.y / steps2};
        V2 p = pp1;
        const int di = (mid.x < pp2.x) ? 1 : -1;
        ScanHalf(p, mid.y, dp1, pp1, pp2, di, dir, n, d);
        ScanHalf(p, pp3.y, dp2, pp2, pp3, di, dir, n, d);
    }
    // RasterLine (Grid3D.cpp:791-811)
    void RasterLine(const float p1[3], const float p2[3])
    {
        const float dir[3] = {fl(p2[0] - p1[0]), fl(p2[1] - p1[1]), fl(p2[2] - p1[2])};
        const int steps = (int)std::max(std::fabs(dir[0]), std::max(std::fabs(dir[1]), std::fabs(dir[2]))) + 1;
        const float dp[3] = {dir[0] / (float)steps, dir[1] / (float)steps, dir[2] / (float)steps};
        float p[3] = {p1[0], p1[1], p1[2]};
        for (int i = 0; i <= steps; i++) {
            Set((int)p[0], (int)p[1], (int)p[2], NODE_BOUND);
            p[0] = fl(p[0] + dp[0]); p[1] = fl(p[1] + dp[1]); p[2] = fl(p[2] + dp[2]);
        }
    }
    // ---- conservative voxelisation: set-up, column and cell test of csrc/fs3d_voxel.h (where the rule is stated), serially -------
    // THIN: the thin shell (shell = 1); a degenerate triangle keeps the conservative treatment inside the shared cell test
    template <bool THIN>
    void VoxelTriangle(const float (&p)[3][3], int t)
    {
        VoxelSetup s;
        if (!voxel_setup<THIN>(p, dimx, dimy, dimz, s)) return;
        const size_t plane = (size_t)dimy * dimz;
        const size_t sa = voxel_sel(s.a, plane, (size_t)dimz, (size_t)1), sb = voxel_sel(s.b, plane, (size_t)dimz, (size_t)1),
                     sd = voxel_sel(s.d, plane, (size_t)dimz, (size_t)1);
        const size_t base = id(s.o[0], s.o[1], s.o[2]);
        for (int ia = 0; ia < s.cnt[0]; ia++)
            for (int ib = 0; ib < s.cnt[1]; ib++) {
                VoxelColumn c;
                if (!voxel_column<THIN>(s, ia, ib, c)) continue;
                for (int k = c.k0; k <= c.k1; k++) {
                    if (!voxel_cell<THIN>(s, c, k)) continue;
                    const size_t cell = base + ia * sa + ib * sb + k * sd;
                    type[cell] = NODE_BOUND;
                    if (!owner.empty() && (owner[cell] < 0 || owner[cell] > t)) owner[cell] = t;
                }
            }
    }

    // Grid3D::Build (Grid3D.cpp:859-903) + FloodFill (:813-857)
    void Build(const Shape3DFrame &fr)
    {
        type.assign((size_t)dimx * dimy * dimz, NODE_IN);
        if (voxels != 0 && voxels != 1) throw std::runtime_error("Shape3D: voxels is 0 (the reference's rasteriser) or 1 (conservative)");
        if (shell != 0 && shell != 1) throw std::runtime_error("Shape3D: shell is 0 (every cell whose box a triangle touches) or 1 (the thin shell of centre crosses)");
        if (shell && voxels != 1) throw std::runtime_error("Shape3D: the thin shell needs the conservative voxelisation (it is a filter inside its overlap test)");
        if (wall_velocity < 0 || wall_velocity > 2) throw std::runtime_error("Shape3D: wall_velocity is 0 (walls at rest), 1 (motion) or 2 (file)");
        if (wall_velocity && voxels != 1) throw std::runtime_error("Shape3D: wall velocities need the conservative voxelisation (the owner of a wall cell is defined by its overlap test)");
        owner.clear();
        if (wall_velocity) {
            if (fr.vx.size() != fr.x.size() || fr.vy.size() != fr.x.size() || fr.vz.size() != fr.x.size()) throw std::runtime_error("Shape3D: one velocity per vertex");
            for (const std::vector<float> *a : {&fr.vx, &fr.vy, &fr.vz})
                for (float v : *a) if (!std::isfinite(v)) throw std::runtime_error("Shape3D: a vertex velocity is not finite");
            owner.assign(type.size(), -1);
            if (&fr != &cur) cur = fr;
        }
        if (voxels == 1)
            for (const std::vector<float> *a : {&fr.x, &fr.y, &fr.z})
                for (float v : *a)
                    if (!(std::fabs(v) <= VOXEL_COORD_MAX))
                        throw std::runtime_error("Shape3D: a vertex coordinate is not finite or exceeds 4096 grid cells in magnitude (conservative voxelisation)");
        for (size_t q = 0; q + 2 < fr.idx.size(); q += 3) {
            const int i1 = fr.idx[q], i2 = fr.idx[q + 1], i3 = fr.idx[q + 2];
            if (voxels == 1) {
                const float p[3][3] = {{fr.x[i1], fr.y[i1], fr.z[i1]}, {fr.x[i2], fr.y[i2], fr.z[i2]}, {fr.x[i3], fr.y[i3], fr.z[i3]}};
                if (shell == 1) VoxelTriangle<true>(p, (int)(q / 3)); else VoxelTriangle<false>(p, (int)(q / 3));
                continue;
            }
            const float p1[3] = {fr.x[i1], fr.y[i1], fr.z[i1]}, p2[3] = {fr.x[i2], fr.y[i2], fr.z[i2]}, p3[3] = {fr.x[i3], fr.y[i3], fr.z[i3]};
            RasterPolygon(p1, p2, p3);
            RasterLine(p1, p2); RasterLine(p1, p3); RasterLine(p3, p2);       // the edges as well, to cover holes
        }
        std::vector<int> queue;
        queue.reserve(3 * 4096);
        auto push = [&](int i, int j, int k) { queue.push_back(i); queue.push_back(j); queue.push_back(k); type[id(i, j, k)] = NODE_OUT; };
        push(0, 0, 0);                                                        // (the reference marks (0,0,0) whatever it was)
        const int nb[18] = {-1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, -1, 0, 0, 1};
        for (size_t cur = 0; cur * 3 < queue.size(); cur++) {
            const int i = queue[cur * 3], j = queue[cur * 3 + 1], k = queue[cur * 3 + 2];
            for (int q = 0; q < 6; q++) {
                const int a = i + nb[3 * q], b = j + nb[3 * q + 1], c = k + nb[3 * q + 2];
                if (a >= 0 && a < dimx && b >= 0 && b < dimy && c >= 0 && c < dimz && type[id(a, b, c)] == NODE_IN) push(a, b, c);
            }
        }
    }
};

// The Node array of the grid `sh` holds: Init's values, then Build's SetData(.., baseT) on NODE_IN / NODE_OUT cells only.
// Third deviation, of a moving run: this is a function of the current grid alone.  The reference's repeated Prepare_CPU(t) keeps
// T = 0 on every cell that once was a wall (Build never writes a NODE_BOUND cell's T and Init runs once); the Node T of a fluid
// cell is read by nothing after the layers have been initialised, so no result differs.
// wallT: the temperature of the NODE_BOUND cells (0: the reference's run); where sh.wall_velocity is set they also carry the
// velocity of the mesh (Shape3D::WallVelocity of the cell's owner, rounded once to FTYPE).
template <typename FTYPE>
void FillShape3DNodes(Grid3D<FTYPE> &g, const Shape3D &sh, double baseT, double wallT = 0)
{
    for (size_t c = 0; c < sh.type.size(); c++) {
        g.type[c] = sh.type[c];
        g.bc_vel[c] = BC_NOSLIP; g.bc_temp[c] = BC_NOSLIP;
        g.vx[c] = 0; g.vy[c] = 0; g.vz[c] = 0;
        g.T[c] = sh.type[c] == NODE_BOUND ? (FTYPE)(float)wallT : (FTYPE)(float)baseT;     // Init: T = 0; Build: SetData(.., baseT) on NODE_IN / NODE_OUT only
        if (sh.type[c] == NODE_BOUND && !sh.owner.empty()) {
            const int k = (int)(c % sh.dimz), j = (int)((c / sh.dimz) % sh.dimy), i = (int)(c / ((size_t)sh.dimz * sh.dimy));
            double u[3];
            sh.WallVelocity(sh.owner[c], i, j, k, u);
            g.vx[c] = (FTYPE)u[0]; g.vy[c] = (FTYPE)u[1]; g.vz[c] = (FTYPE)u[2];
        }
    }
}

// Grid3D(dx,dy,dz,baseT) + LoadFromFile + Prepare_CPU(0) for a Shape3D input (FluidSolver3D.cpp:121-145)
template <typename FTYPE>
void LoadShape3D(Grid3D<FTYPE> &g, Shape3D &sh, const std::string &path, double dx, double dy, double dz, double baseT, bool align, int voxels = 0,
                 int wall_velocity = 0, double wallT = 0, int shell = 0)
{
    sh.voxels = voxels;
    sh.shell = shell;
    sh.wall_velocity = wall_velocity;
    sh.Load(path, dx, dy, dz, align);
    g.Resize(sh.dimx, sh.dimy, sh.dimz);
    g.dx = dx; g.dy = dy; g.dz = dz; g.baseT = baseT;
    FillShape3DNodes(g, sh, baseT, wallT);
}

}  // namespace fs3d
