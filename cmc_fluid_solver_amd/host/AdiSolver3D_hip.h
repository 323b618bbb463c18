// C++ host side above the C ABI (include/fs3d.h): the reference's solver interface for this path,
// re-shaped around libfs3d_hip.so.  A driver written against the reference's Solver3D
// (Solver3D.h:24-49) / AdiSolver3D (AdiSolver3D.h:61-70) calls the same methods with the same
// argument meaning: Init, UpdateBoundaries, TimeStep, GetLayer; failures surface as
// std::runtime_error exactly where the reference throws (gpuSafeCall, GPUplan.cpp:173-193;
// "Error is too big!", AdiSolver3D.cpp:371-374).
//
// Header-only; link with -lfs3d_hip.  No CPU fallback exists: without the library or a GPU
// every call throws.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/fs3d.h"

namespace fs3d {

// Geometry.h:29-43
enum NodeType : uint8_t { NODE_IN = 0, NODE_OUT = 1, NODE_BOUND = 2, NODE_VALVE = 3 };
enum BCtype : uint8_t { BC_NOSLIP = 0, BC_FREE = 1 };

// Geometry.h:538-562
template <typename FTYPE>
struct FluidParams {
    FTYPE v_T, v_vis, t_vis, t_phi;
    FluidParams() : v_T(1), v_vis(0), t_vis(0), t_phi(0) {}
    FluidParams(double Re, double Pr, double lambda)
        : v_T(1.0), v_vis((FTYPE)(1.0 / Re)), t_vis((FTYPE)(1.0 / (Re * Pr))), t_phi((FTYPE)((lambda - 1) / (lambda * Re))) {}
    FluidParams(double vis, double rho, double R, double k, double cv)
        : v_T((FTYPE)R), v_vis((FTYPE)(vis / rho)), t_vis((FTYPE)(k / (rho * cv))), t_phi((FTYPE)(vis / (rho * cv))) {}
};

// The part of Grid3D (Grid3D.h:95-200) the solver consumes: dims, spacing and the Node array
// (type, bc_vel, bc_temp, v, T; Grid3D.h:73-88) as structure-of-arrays.
template <typename FTYPE>
struct Grid3D {
    int dimx = 0, dimy = 0, dimz = 0;
    double dx = 0, dy = 0, dz = 0, baseT = 0;
    std::vector<uint8_t> type, bc_vel, bc_temp;
    std::vector<FTYPE> vx, vy, vz, T;
    void Resize(int nx, int ny, int nz)
    {
        dimx = nx; dimy = ny; dimz = nz;
        const size_t n = (size_t)nx * ny * nz;
        type.assign(n, NODE_OUT); bc_vel.assign(n, BC_NOSLIP); bc_temp.assign(n, BC_NOSLIP);
        vx.assign(n, 0); vy.assign(n, 0); vz.assign(n, 0); T.assign(n, 0);
    }
    size_t Index(int i, int j, int k) const { return ((size_t)i * dimy + j) * dimz + k; }   // TimeLayer3D.h:256-259
    NodeType GetType(int i, int j, int k) const { return (NodeType)type[Index(i, j, k)]; }
    // Node::SetBound, Grid3D.h:80-87
    void SetBound(int i, int j, int k, BCtype bv, BCtype bt, FTYPE ux, FTYPE uy, FTYPE uz, FTYPE t, NodeType nt = NODE_BOUND)
    {
        const size_t id = Index(i, j, k);
        type[id] = nt; bc_vel[id] = bv; bc_temp[id] = bt; vx[id] = ux; vy[id] = uy; vz[id] = uz; T[id] = t;
    }
};

template <typename FTYPE>
class AdiSolver3D {
public:
    AdiSolver3D() = default;
    AdiSolver3D(const AdiSolver3D &) = delete;
    AdiSolver3D &operator=(const AdiSolver3D &) = delete;
    ~AdiSolver3D() { if (ctx_) fs3d_destroy(ctx_); }

    // AdiSolver3D::Init (AdiSolver3D.cpp:166-268) + CreateSegments (:553-562) + the cur layer's
    // CopyFromGrid constructor (TimeLayer3D.h:1076-1090).  x0/x1 select this process's x-slab.
    void Init(int device, const Grid3D<FTYPE> &grid, const FluidParams<FTYPE> &params, int x0 = 0, int x1 = -1)
    {
        if (x1 < 0) x1 = grid.dimx;
        grid_ = &grid;
        const fs3d_precision prec = sizeof(FTYPE) == 4 ? FS3D_F32 : FS3D_F64;
        fs3d_status st = fs3d_create(&ctx_, device, prec, x1 - x0, grid.dimy, grid.dimz, grid.dx, grid.dy, grid.dz, x0, grid.dimx);
        if (st != FS3D_OK) throw std::runtime_error(std::string("fs3d_create: ") + fs3d_last_error(nullptr));
        chk(fs3d_set_params(ctx_, params.v_T, params.v_vis, params.t_vis, params.t_phi));
        chk(fs3d_upload_nodes(ctx_, grid.type.data(), grid.bc_vel.data(), grid.bc_temp.data(), grid.vx.data(), grid.vy.data(),
                              grid.vz.data(), grid.T.data(), numSegs));
        chk(fs3d_init_layers_from_nodes(ctx_));
        dimx = x1 - x0; dimy = grid.dimy; dimz = grid.dimz;
        slab_ = x0 != 0 || x1 != grid.dimx;
    }
    // multi-GPU: join the RCCL group (one process per GPU); id = 128-byte ncclUniqueId from UniqueId() on rank 0
    static void UniqueId(void *id128) { if (fs3d_comm_unique_id(id128) != FS3D_OK) throw std::runtime_error("fs3d_comm_unique_id failed"); }
    void JoinGroup(const void *id128, int rank, int nranks) { chk(fs3d_comm_init(ctx_, id128, rank, nranks)); slab_ = true; }
    // multi-GPU, one process (the reference's GPUplan mode, "GPU n"): one solver per slab, each driven by its own host thread,
    // joined by an in-process group; every collective call (TimeStep, ...) is then made by all the threads
    static void *CreateLocalGroup(int nranks) { void *g = nullptr; if (fs3d_local_group_create(nranks, &g) != FS3D_OK) throw std::runtime_error("fs3d_local_group_create failed"); return g; }
    static void DestroyLocalGroup(void *g) { fs3d_local_group_destroy(g); }
    void JoinLocalGroup(void *group, int rank) { chk(fs3d_comm_init_local(ctx_, group, rank)); slab_ = true; }

    // AdiSolver3D::CreateSegments again, for a grid whose walls have moved (same dims): the device tables are rebuilt by kernels,
    // the layers are kept.  A solver with a slab range or in a group (fs3d_update_nodes_slab): `grid` is the GLOBAL grid, every
    // rank is given the same one between the same two steps and rebuilds the tables of its own planes; no rank waits for another.
    void UpdateGrid(const Grid3D<FTYPE> &grid)
    {
        grid_ = &grid;
        chk((slab_ ? fs3d_update_nodes_slab : fs3d_update_nodes)(ctx_, grid.type.data(), grid.bc_vel.data(), grid.bc_temp.data(), grid.vx.data(), grid.vy.data(),
                              grid.vz.data(), grid.T.data(), numSegs));
    }
    // The same for a grid that is the extrusion of a 2D grid (Grid3D::Prepare2D, Grid3D.cpp:608-668): g2 as it stands after
    // g2.Prepare(t) is extruded on the device -- its cell types and three floats per column travel, no 3D node array is built or
    // copied on the host.  G2 = fs3d::Grid2D (host/Shape2D.h); dz, depth, depth_var as ExtrudeShape2D takes them, baseT the grid's
    // of Init.  The host Grid3D given to Init is NOT kept current by this call: only its dims and baseT are read afterwards.
    // On a slab or in a group as UpdateGrid: g2 is the global 2D grid (fs3d_update_nodes_shape2d_slab).
    template <typename G2>
    void UpdateGridExtruded(const G2 &g2, double dz, double depth, double depth_var)
    {
        if (g2.dimx != grid_->dimx || g2.dimy != grid_->dimy) throw std::runtime_error("UpdateGridExtruded: the 2D grid does not have the 3D grid's dims");
        chk((slab_ ? fs3d_update_nodes_shape2d_slab : fs3d_update_nodes_shape2d)(ctx_, g2.cell.data(), g2.velx.data(), g2.vely.data(), g2.T.data(), dz, depth, depth_var, grid_->baseT, numSegs));
    }
    // The same for the grid of a Shape3D mesh (Grid3D::Prepare3D_Shape, Grid3D.cpp:905-946): the sub-frame's vertices in grid
    // coordinates (Shape3D::SubFrame(t), host/Shape3D.h) and the triangle indices travel, the mesh is voxelised and flood-filled on
    // the device.  As with UpdateGridExtruded the host Grid3D given to Init is NOT kept current: its dims and baseT are read.
    // On a slab or in a group as UpdateGrid: the vertices are in GLOBAL grid coordinates and every rank is given the same mesh
    // (fs3d_update_nodes_shape3d_slab, fs3d_update_nodes_shape3d_vel_slab); each voxelises and fills the global grid for itself.
    void UpdateGridShape3D(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &z, const std::vector<int> &idx)
    {
        if (x.size() != y.size() || x.size() != z.size()) throw std::runtime_error("UpdateGridShape3D: x, y, z differ in length");
        static const int none = 0;
        chk((slab_ ? fs3d_update_nodes_shape3d_slab : fs3d_update_nodes_shape3d)(ctx_, x.data(), y.data(), z.data(), (int)x.size(), idx.empty() ? &none : idx.data(), (int)(idx.size() / 3),
                                      grid_->baseT, numSegs));
    }
    // The same with walls that carry the mesh's velocity and a temperature (fs3d_update_nodes_shape3d_vel; conservative voxelisation
    // only: SetMeshVoxels(1) first): wx, wy, wz the vertex velocities of the sub-frame (Shape3D::SubFrameVelocity), wallT the
    // temperature of the NODE_BOUND cells.  Zero velocities and wallT = 0 give the grid of the overload above.
    void UpdateGridShape3D(const std::vector<float> &x, const std::vector<float> &y, const std::vector<float> &z, const std::vector<float> &wx,
                           const std::vector<float> &wy, const std::vector<float> &wz, const std::vector<int> &idx, double wallT)
    {
        if (x.size() != y.size() || x.size() != z.size()) throw std::runtime_error("UpdateGridShape3D: x, y, z differ in length");
        if (x.size() != wx.size() || x.size() != wy.size() || x.size() != wz.size()) throw std::runtime_error("UpdateGridShape3D: one velocity per vertex");
        static const int none = 0;
        chk((slab_ ? fs3d_update_nodes_shape3d_vel_slab : fs3d_update_nodes_shape3d_vel)(ctx_, x.data(), y.data(), z.data(), wx.data(), wy.data(), wz.data(), (int)x.size(),
                                          idx.empty() ? &none : idx.data(), (int)(idx.size() / 3), grid_->baseT, wallT, numSegs));
    }
    // FS3D_OPT_MESH_VOXELS for the UpdateGridShape3D calls that follow: 0 the reference's rasteriser, 1 the conservative
    // voxelisation (Shape3D::voxels of host/Shape3D.h has the same values)
    void SetMeshVoxels(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_MESH_VOXELS, mode)); }
    // FS3D_OPT_MESH_SHELL for the same calls: 0 the conservative shell as it is, 1 its thin subset (needs SetMeshVoxels(1))
    void SetMeshShell(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_MESH_SHELL, mode)); }
    // FS3D_OPT_OUTPUT_FILTER for the GetLayer / GetLayerRows calls that follow: 0 the reference's point sample, 1 the mean over the
    // NODE_IN cells of every sample's box of source cells (the point sample where a box holds none).  While it is not 0 the calls
    // of a slab solver throw (FS3D_ERR_UNSUPPORTED)
    void SetOutputFilter(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_FILTER, mode)); }
    // FS3D_OPT_OUTPUT_SLABS: 1 = on a slab of a group GetLayerRows / GetLayerDev take the filter and vector options, as one collective call of
    // all slabs (every rank between the same two steps, with the same output dims and options); 0 (default): they refuse them on a slab
    void SetOutputSlabs(int on) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_SLABS, on)); }
    // FS3D_OPT_OUTPUT_VECTOR for the same calls: 0 resVel holds the velocity, 1 the vorticity (central differences on the NODE_IN
    // cells whose six neighbours are no NODE_OUT cells, 99999 on NODE_OUT cells, 0 elsewhere); slab solvers throw as above
    void SetOutputVector(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_VECTOR, mode)); }
    // FS3D_OPT_OUTPUT_GRADIENT for the same calls: 1 resVel holds the invariants of the velocity gradient of the sampled layer --
    // div u, the Q criterion and the strain rate S:S, on the cells that carry a vorticity, 99999 on NODE_OUT cells, 0 elsewhere --,
    // accepted and refused where SetOutputVector(1) is; 2 their time mean (needs SetOutputSource(1) and a window accumulated with
    // SetTimeStatsGradients(1)); 0 off.  With SetOutputVector(1) as well the calls throw (FS3D_ERR_INVALID)
    void SetOutputGradient(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_GRADIENT, mode)); }
    // FS3D_OPT_TIME_STATS_GRAD: 1 -- with SetTimeStats(1 or 2) every accumulated step also adds div u, Q and S:S of its result to
    // per-cell sums (the cells that carry them at that step), 0 -- off, those sums are freed.  EVERY call opens a new window.  A
    // single-GPU solver only: a slab solver throws (FS3D_ERR_UNSUPPORTED)
    void SetTimeStatsGradients(int on) { chk(fs3d_set_option(ctx_, FS3D_OPT_TIME_STATS_GRAD, on)); }
    // FS3D_OPT_OUTPUT_WALL for the same calls: 1 resVel holds the wall shear stress vector of the sampled layer on the wall cells
    // that carry one (a wall cell with a fluid neighbour on a line the solver closes there), 2 its magnitude, the wall heat flux and
    // the exposed area, 99999 on NODE_OUT cells, 0 elsewhere; with SetOutputFilter(1) the mean over the carriers of a box; 3 the
    // time mean of the vector, 4 the time-averaged magnitude (TAWSS), the mean heat flux and the oscillatory shear index (both
    // need SetOutputSource(1) and a window accumulated with SetTimeStatsWall(1)); 0 off.  With SetOutputVector(1) or a non-zero
    // SetOutputGradient the calls throw (FS3D_ERR_INVALID); a slab solver throws (FS3D_ERR_UNSUPPORTED)
    void SetOutputWall(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_WALL, mode)); }
    // FS3D_OPT_TIME_STATS_WALL: 1 -- with SetTimeStats(1 or 2) every accumulated step also adds the wall shear stress, its
    // magnitude and the wall heat flux of its result to per-cell sums (the carriers of that step), 0 -- off, those sums are freed.
    // EVERY call opens a new window.  A single-GPU solver only: a slab solver throws (FS3D_ERR_UNSUPPORTED)
    void SetTimeStatsWall(int on) { chk(fs3d_set_option(ctx_, FS3D_OPT_TIME_STATS_WALL, on)); }
    // FS3D_OPT_TIME_STATS: 1 -- from now on every TimeStep that succeeds adds its result to per-cell sums on the device (the cells
    // that are NODE_IN at that step), 2 -- and its squares, 0 -- off, the sums are freed.  EVERY call opens a new window.  Works on
    // a slab solver as on a single one (a cell asks nothing of a neighbour)
    void SetTimeStats(int mode) { chk(fs3d_set_option(ctx_, FS3D_OPT_TIME_STATS, mode)); }
    // FS3D_OPT_TIME_STATS_CROSS: 1 -- with SetTimeStats(2) every accumulated step also adds the six products uv, uw, vw, uT, vT, wT to
    // per-cell sums (the Reynolds stresses and the turbulent heat fluxes of SetOutputMoment), 0 -- off, those sums are freed.  EVERY
    // call opens a new window
    void SetTimeStatsCross(int on) { chk(fs3d_set_option(ctx_, FS3D_OPT_TIME_STATS_CROSS, on)); }
    // FS3D_OPT_TIME_STATS_EVERY: of the successful TimeSteps of a window the 1st, (k + 1)th, (2k + 1)th, .. are accumulated, on the
    // others nothing runs; k from 1 (the default) to 2^20.  EVERY call opens a new window
    void SetTimeStatsEvery(int k) { chk(fs3d_set_option(ctx_, FS3D_OPT_TIME_STATS_EVERY, k)); }
    // FS3D_OPT_OUTPUT_MOMENT, read while SetOutputSource(2): 0 the four variances, 1 the Reynolds stresses u'v', u'w', v'w' in resVel
    // and the turbulent kinetic energy in resT, 2 the heat fluxes u'T', v'T', w'T' in resVel and the variance of T in resT.  With 1 or
    // 2 the calls throw (FS3D_ERR_INVALID) without SetTimeStats(2) and SetTimeStatsCross(1), and with SetOutputVector(1)
    void SetOutputMoment(int moment) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_MOMENT, moment)); }
    // FS3D_OPT_OUTPUT_SOURCE for the GetLayer / GetLayerRows calls that follow: 0 `next` as always, 1 the time mean of the window,
    // 2 its variance (needs SetTimeStats(2)), 3 the fluid fraction (in T; the velocity is 0).  The calls throw (FS3D_ERR_INVALID)
    // for a source the mode does not hold and for a window without a step; filter and vector apply to the statistic layer
    void SetOutputSource(int source) { chk(fs3d_set_option(ctx_, FS3D_OPT_OUTPUT_SOURCE, source)); }
    // FS3D_OPT_FRESH_CELLS: with it on, every UpdateGrid* call of a single-GPU solver keeps the node types of the geometry it
    // replaces, and FillFreshCells, called directly after the update and before UpdateBoundaries, gives every cell of `cur` that
    // the update turned NODE_IN the mean of its fluid neighbours (fs3d_fill_fresh_cells; no reference
    // counterpart).  info: fresh cells, filled, rounds, left unfilled.  A slab of a group throws unless SetFreshCellsSlabs(true) was
    // called on every slab; a lone slab of a larger grid, in no group, always throws.
    void SetFreshCells(bool on) { chk(fs3d_set_option(ctx_, FS3D_OPT_FRESH_CELLS, on ? 1 : 0)); }
    // FS3D_OPT_FRESH_CELLS_SLABS, for a solver that has joined a group (JoinLocalGroup, JoinGroup): with SetFreshCells(true) the
    // UpdateGrid* calls of the slab keep the node types of its own planes, and FillFreshCells becomes a collective call -- every slab
    // of the group makes it between the same two steps, the slabs exchange a plane of fields and tags per round, and the planes of
    // every slab end with the bits the single-GPU fill leaves in them.  info then counts the slab's own fresh, filled and unfilled
    // cells (their sums over the slabs are the single-GPU numbers); the rounds are the group's, the same on every slab.
    void SetFreshCellsSlabs(bool on) { chk(fs3d_set_option(ctx_, FS3D_OPT_FRESH_CELLS_SLABS, on ? 1 : 0)); }
    void FillFreshCells(long long info[4]) { chk(fs3d_fill_fresh_cells(ctx_, FS3D_LAYER_CUR, 0, info)); }
    // Solver3D::ClearOutterCells (Solver3D.cpp:41-44), on `next` as there and on `cur`: a cell that turns NODE_IN with the next
    // geometry starts from (0, 0, 0, baseT) in both
    void ClearOutterCells()
    {
        chk(fs3d_clear_outer_cells(ctx_, FS3D_LAYER_NEXT, grid_->baseT));
        chk(fs3d_clear_outer_cells(ctx_, FS3D_LAYER_CUR, grid_->baseT));
    }
    void UpdateBoundaries() { chk(fs3d_update_boundaries(ctx_)); }                        // AdiSolver3D.cpp:286-304
    // AdiSolver3D::TimeStep (AdiSolver3D.cpp:306-391); throws where the reference throws
    void TimeStep(FTYPE dt, int num_global, int num_local, bool computeError)
    {
        fs3d_status st = fs3d_time_step(ctx_, dt, num_global, num_local, computeError ? 1 : 0, &diffError);
        if (st != FS3D_OK) throw std::runtime_error(fs3d_last_error(ctx_));
    }
    // Solver3D::GetLayer (Solver3D.cpp:21-25): v = interleaved x,y,z (Vec3D), T = double
    void GetLayer(FTYPE *v, double *T, int outdimx = 0, int outdimy = 0, int outdimz = 0) { chk(fs3d_get_layer(ctx_, v, T, outdimx, outdimy, outdimz)); }
    // the same on an x-slab of a group: v / T are the arrays of the WHOLE output grid (0 = the grid's global dim), this slab writes
    // the rows [rows[0], rows[1]) whose source plane it owns -- disjoint over the slabs, together [0, outdimx)
    void GetLayerRows(FTYPE *v, double *T, int outdimx, int outdimy, int outdimz, int rows[2]) { chk(fs3d_get_layer_rows(ctx_, v, T, outdimx, outdimy, outdimz, rows)); }
    // cur layer on the host (ScalarField3D(CPU, field) copy constructor, TimeLayer3D.h:358-383)
    void DownloadCur(FTYPE *u, FTYPE *v, FTYPE *w, FTYPE *T) { chk(fs3d_download_layer(ctx_, FS3D_LAYER_CUR, u, v, w, T)); }
    // device time per event class since EnableTiming(true): 0 sweeps Z, 1 sweeps Y, 2 sweeps X, 3 everything else
    void EnableTiming(bool on) { chk(fs3d_enable_timing(ctx_, on ? 1 : 0)); }
    void Timings(float ms[4], int count[4]) { chk(fs3d_last_step_timing(ctx_, ms, count)); }
    // the same under the reference Profiler's event names (Common/Profiler.h; AdiSolver3D.cpp:297-367, 555-680)
    void ProfilerEvents(const char *names[FS3D_N_EVENTS], float ms[FS3D_N_EVENTS], int count[FS3D_N_EVENTS]) { chk(fs3d_profiler_events(ctx_, names, ms, count)); }
    double EvalDivError() { double e = 0; chk(fs3d_eval_div_error(ctx_, FS3D_LAYER_NEXT, &e, nullptr)); return e; }

    fs3d_ctx *ctx() const { return ctx_; }              // for C-ABI calls the class does not wrap

    double diffError = 0.0;
    int numSegs[3] = {0, 0, 0};
    int dimx = 0, dimy = 0, dimz = 0;

private:
    void chk(fs3d_status st) { if (st != FS3D_OK) throw std::runtime_error(fs3d_last_error(ctx_)); }
    fs3d_ctx *ctx_ = nullptr;
    const Grid3D<FTYPE> *grid_ = nullptr;
    bool slab_ = false;                                 // Init with a slab range, or a member of a group: the geometry updates take the slab entries
};

}  // namespace fs3d
