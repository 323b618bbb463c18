// Command-line driver: the reference's FluidSolver3D main (FluidSolver3D/FluidSolver3D.cpp:60-330) on top of
// libfs3d_hip.so.   fs3d_run <input data> <output prefix> <config> [align] [GPU [n]] [double] [moving [--host-extrusion] [--time-geometry]] [moving-mesh [--host-voxels | --slab-voxels] [--time-geometry] [--time-both]] [--time-output] [--steps N] [--same-device] [--grid-only FILE [--grid-time T]] [--watertight [--thin-shell] [--wall-velocity motion|file]] [--wall-temperature T] [--fresh-cells | --slab-fresh-cells] [--output-filter point|box] [--time-stats mean|variance] [--time-covariances] [--time-stats-every K]
//   * reads the config (host/Config.h) and a Shape2D, Shape3D or SeaNetCDF geometry (host/Shape2D.h, Shape3D.h, SeaNetCDF.h), prints the grid summary lines
//     the reference prints ("Grid = X x Y x Z", "NODE_IN points = ..."),
//   * runs the same loop: dt = cycle length / (frames * time_steps), UpdateBoundaries + TimeStep per step with the
//     divergence error every 10th step and on the last one, "err = ..." and the progress line per step,
//   * writes <output prefix>_res.nc through host/NetCDF3.h every out_time_steps steps (GetLayer).
// `transpose`, `decompose`, `blocking n` of the reference are accepted and ignored (backend tuning switches); `CSV`
// switches the closing timing table to the reference's comma-separated form.
// `moving` (in_fmt Shape2D; one GPU, or GPU n --same-device: run_slabs below): the walls follow the frames of the input -- per step grid2D->Prepare(t), the extrusion and
//   CreateSegments on the device (UpdateGridExtruded: the 2D grid travels, the node arrays are written by a kernel), UpdateBoundaries,
//   TimeStep, the output, ClearOutterCells: the loop of the reference's 2D driver (FluidSolver2D.cpp:130-133) with the 3D classes'
//   mechanism (AdiSolver3D.cpp:382-385, Solver3D.cpp:41-44).
//   --host-extrusion: the extrusion on the host (ExtrudeShape2D into the Grid3D, then UpdateGrid with its seven arrays) -- the same
//   results bit for bit; kept for A/B timing and as the checker of the device extrusion.
//   --time-geometry: one more line after the timing table, the host clock per step around Prepare, the host extrusion and the update call.
// `moving-mesh` (in_fmt Shape3D; one GPU, or GPU n with --host-voxels or --slab-voxels: run_slabs below): the same loop for a triangle mesh per frame -- per step Shape3D::SubFrame(t) (the
//   interpolation of Grid3D::Prepare3D_Shape, Grid3D.cpp:905-946), then the voxelisation, the flood fill and CreateSegments on the
//   device (UpdateGridShape3D: the vertices travel).  The frame counter of the progress line stays 0, as Grid3D::GetFrame gives it
//   for a Shape3D input.  `moving` keeps its meaning: Shape2D inputs only.
//   --host-voxels: Shape3D::Prepare(t) on the host (rasteriser and flood fill), then UpdateGrid with the seven arrays -- the same
//   results bit for bit; kept for A/B timing and as the checker of the device voxeliser.
//   --slab-voxels (GPU n, n > 1): the device path on x-slabs -- rank 0 computes SubFrame(t) (and the vertex velocities) once, every
//   rank voxelises and fills the GLOBAL grid on its own device and builds the tables of its planes (UpdateGridShape3D: the slab
//   entries fs3d_update_nodes_shape3d_slab / _vel_slab).  --watertight, --wall-velocity and --wall-temperature as on one GPU.
//   --watertight (in_fmt Shape3D, with or without moving-mesh): the conservative voxelisation instead of the reference's rasteriser
//   (Shape3D::voxels = 1 on the host, FS3D_OPT_MESH_VOXELS = 1 on the device) for the first geometry and for every update alike: a
//   closed mesh keeps its NODE_IN cells at every time; the shell is thicker, so the fluid volume is smaller.
//   --thin-shell (needs --watertight): of the conservative shell only the cells whose centre cross a triangle meets (Shape3D::shell = 1
//   on the host, FS3D_OPT_MESH_SHELL = 1 on the device) -- still closed for the fill, about 0.55 of the wall cells, so more fluid; for the
//   first geometry, every moving-mesh update (device, --host-voxels, --slab-voxels) and --grid-only alike.
//   --wall-velocity motion|file (in_fmt Shape3D, needs --watertight): the NODE_BOUND cells carry the velocity of the mesh -- of the
//   cell's owner triangle at the projection of the cell's centre (host/Shape3D.h WallVelocity) -- in the first geometry and in every
//   moving-mesh update (UpdateGridShape3D with velocities: fs3d_update_nodes_shape3d_vel), so a moving wall pushes the fluid.
//   `motion`: the vertices' displacement per frame over the frame's duration; `file`: the velocity columns of the input,
//   interpolated as the reference does and taken as they are.  With --host-voxels the host loader computes the same arrays, bit for bit.
//   --wall-temperature T (in_fmt Shape3D): T of the NODE_BOUND cells instead of 0; a moving-mesh run on the device needs --watertight for it.
//   --time-both: a measurement run -- every step makes the geometry through BOTH paths, the word's own last (same tables either way),
//   and one more line gives, per call after 3 warm-up steps, median (min - max) of the host clock around each path, the device
//   time of the device path (fs3d_last_update_device_ms), and the host clock around UpdateBoundaries + TimeStep, synchronised.
// --fresh-cells (with moving or moving-mesh, one GPU): directly after every geometry update and before UpdateBoundaries, the cells of
//   `cur` that the update turned NODE_IN take the mean of their fluid neighbours (FS3D_OPT_FRESH_CELLS, FillFreshCells)
//   instead of starting from the values of the wall or the outside they were.  Either way of making the
//   geometry (device, --host-extrusion / --host-voxels) goes through an update entry, so both work, with the same results.  One
//   more line after the timing table: "Fresh cells: <fresh> in <updates> updates, <filled> filled, at most <rounds> rounds".
//   Refused with GPU n (use --slab-fresh-cells), with --time-both (two updates per step) and without a moving word.
// --slab-fresh-cells: --fresh-cells that also runs with GPU n, wherever this driver moves a geometry on x-slabs (moving --same-device,
//   moving-mesh --host-voxels, moving-mesh --slab-voxels): every rank sets FS3D_OPT_FRESH_CELLS and FS3D_OPT_FRESH_CELLS_SLABS and
//   fills directly after its update and before UpdateBoundaries -- a collective call, the slabs exchange a plane of fields and round
//   tags per round.  The results and the `Fresh cells:` line (sums over the ranks, the group's rounds) equal the single-GPU run's.
//   With one GPU it is --fresh-cells.
// --output-filter point|box: `box` calls SetOutputFilter(1) before the loop -- every sample of a record is the mean over the NODE_IN cells of
//   its box of source cells instead of one cell of it (FS3D_OPT_OUTPUT_FILTER; walls and the outside show only where a box holds no
//   fluid); `point`, the default, is the reference's sample.  With an output grid at least as fine as the grid the two are the same
//   bytes.  `box` is refused with GPU n, n > 1, when the arguments are read: a box can straddle the cut between two x-slabs.
//   (The vorticity, FS3D_OPT_OUTPUT_VECTOR, has no word: the result file's variables are the reference's u, v, w, T.)
// --time-stats mean|variance: SetTimeStats(1 | 2) before the loop -- every time step adds its result to per-cell sums on the device
//   (FS3D_OPT_TIME_STATS) -- and after the loop one more file, <prefix>_stats.nc, with the header of _res.nc: record 0 is the time mean of
//   u, v, w, T over the steps of the run, with `variance` record 1 is their variance, the last record is the fluid fraction (the share of the
//   steps a cell was NODE_IN, in T; u = v = w = 0).  Each record is taken by GetLayer (GPU n: GetLayerRows, as the normal records are) at
//   the config's output dims with SetOutputSource(1 | 2 | 3), cells that are NODE_OUT at the end carry 99999, --output-filter box applies
//   to them as to every record; the record axis of that file counts statistics, not time.  _res.nc and every other line are those of
//   the run without the word.  The last line: "Time statistics: <N> steps, mean[, variance] in <file>".  A run of no step (--steps 0)
//   has no window to read: no file is written and the line is "Time statistics: 0 steps, no file".
// --time-covariances, with --time-stats variance (else refused when the arguments are read: "--time-covariances: needs --time-stats
//   variance"): SetTimeStatsCross(1) before the loop -- every accumulated step also adds the six products uv, uw, vw, uT, vT, wT to
//   per-cell sums (FS3D_OPT_TIME_STATS_CROSS) -- and <prefix>_stats.nc holds five records, in this order: mean, variance, Reynolds
//   stresses (u'v' in u, u'w' in v, v'w' in w, the turbulent kinetic energy in T), turbulent heat flux (u'T' in u, v'T' in v, w'T'
//   in w, the variance of T in T), fluid fraction; the two new ones are source 2 with SetOutputMoment(1 | 2), taken as the others.
//   The last line then reads "Time statistics: <N> steps, mean, variance, covariances in <file>".
// --time-stats-every K, K an integer from 1 to 1048576 (else refused when the arguments are read): SetTimeStatsEvery(K) before the
//   loop -- of the time steps of the run the 1st, (K + 1)th, (2K + 1)th, .. are accumulated and nothing runs on the others
//   (FS3D_OPT_TIME_STATS_EVERY); <N> of the last line counts the accumulated steps.  Without --time-stats it has no effect.
//   Without the two words every file and every print is that of --time-stats alone.
// --time-output: one closing line, the host clock per output record around the GetLayer call (GPU n: rank 0's call and the barrier that
//   completes the record) and around AppendLayer, with the number of records.
// There is no CPU backend here: without a GPU the run stops with the library's error.
// --grid-only FILE: build the grid, dump it (dims, type, bc_vel, bc_temp, vx, vy, vz, T as raw arrays) and exit
//   without touching the GPU -- used by the CPU tests to compare the C++ loader with its Python twin.
//   --grid-time T: the grid the moving loop uses at time T (Shape2D: load, Prepare(T), extrude again; Shape3D: Prepare(T)) instead of the one of time 0.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "AdiSolver3D_hip.h"
#include "Config.h"
#include "NetCDF3.h"
#include "Shape2D.h"
#include "Shape3D.h"
#include "SeaNetCDF.h"
#include "GridImage.h"

// what the time loop and the result header need from the geometry (Grid3D::GetFramesNum / GetCycleLength / GetFrame / GetBBox)
struct RunGeom {
    int frames = 1;
    double length = 0;
    float bbox[6] = {0, 0, 0, 0, 0, 0};
    const fs3d::Grid2D *g2 = nullptr;                 // Shape2D: frames in time; Shape3D / SeaNetCDF: frame 0 throughout (Grid3D.cpp:322-328)
    const fs3d::DepthInfo3D *depths = nullptr;        // SeaNetCDF: the depth map (`d` output variable), x / y in degrees
    int GetFrame(double t) const { return g2 ? g2->GetFrame(t) : 0; }
};

// the words after <config file>, as main's argument loop finds them
struct RunOptions {
    bool align = false, dbl = false, csv = false, same_device = false, grid_images = false, watertight = false, thin_shell = false;
    bool moving = false, host_extrusion = false, moving_mesh = false, host_voxels = false, slab_voxels = false, time_geometry = false, time_both = false, time_output = false;
    double grid_time = -1, wall_T = 0;
    int wall_velocity = 0;                             // 0: walls at rest; 1: motion; 2: file (Shape3D::wall_velocity)
    bool has_wall_T = false, fresh_cells = false, slab_fresh_cells = false, output_box = false;
    int time_stats = 0;                                // --time-stats: 0 none, 1 mean, 2 mean and variance (FS3D_OPT_TIME_STATS)
    bool time_cov = false;                             // --time-covariances (FS3D_OPT_TIME_STATS_CROSS; needs time_stats 2)
    long time_every = 1;                               // --time-stats-every K (FS3D_OPT_TIME_STATS_EVERY)
    int nslabs = 1, device = 0;
    long max_steps = -1;
    std::string grid_only;
};

template <typename FTYPE>
static int run_slabs(fs3d::Grid3D<FTYPE> &grid, fs3d::Grid2D &g2, fs3d::Shape3D &sh3, const RunGeom &geo, const std::string &prefix,
                     const fs3d::Config &cfg, const RunOptions &o);

// --time-stats: the records of <prefix>_stats.nc, in order, each a source and a moment (FS3D_OPT_OUTPUT_SOURCE: 1 mean, 2 second
// moments, 3 fluid fraction; FS3D_OPT_OUTPUT_MOMENT: 0 variance, 1 stresses, 2 heat flux)
struct StatsRecord { int source, moment; };
static std::vector<StatsRecord> stats_records(const RunOptions &o)
{
    if (o.time_stats != 2) return {{1, 0}, {3, 0}};
    if (!o.time_cov) return {{1, 0}, {2, 0}, {3, 0}};
    return {{1, 0}, {2, 0}, {2, 1}, {2, 2}, {3, 0}};
}
// the window's options, before the loop
template <class Solver>
static void set_time_stats(Solver &solver, const RunOptions &o)
{
    solver.SetTimeStats(o.time_stats);
    if (o.time_cov) solver.SetTimeStatsCross(1);
    if (o.time_every > 1) solver.SetTimeStatsEvery((int)o.time_every);
}
// steps: the time steps of the run; the line names the accumulated ones, the 1st, (K + 1)th, .. of them
static void print_stats_line(long steps, const RunOptions &o, const std::string &file)
{
    if (steps > 0) std::printf("Time statistics: %ld steps, mean%s%s in %s\n", (steps + o.time_every - 1) / o.time_every,
                               o.time_stats == 2 ? ", variance" : "", o.time_cov ? ", covariances" : "", file.c_str());
    else std::printf("Time statistics: 0 steps, no file\n");
}

template <typename FTYPE>
static int run(const std::string &data, const std::string &prefix, const fs3d::Config &cfg, const RunOptions &o)
{
    if (o.moving && cfg.in_fmt != "Shape2D") throw std::runtime_error("moving: only in_fmt Shape2D inputs move (this one is " + cfg.in_fmt + ")");
    if (o.moving && o.nslabs > 1 && !o.same_device)
        throw std::runtime_error("moving: single GPU only, or GPU n with --same-device (this driver runs a moving Shape2D geometry on x-slabs of one device only; "
                                 "over several devices use fs3d_update_nodes_shape2d_slab through AdiSolver3D::UpdateGridExtruded)");
    if (o.host_extrusion && !o.moving) throw std::runtime_error("--host-extrusion: only with moving (it selects where a moving geometry is extruded)");
    if (o.moving_mesh && cfg.in_fmt != "Shape3D") throw std::runtime_error("moving-mesh: only in_fmt Shape3D inputs are meshes (this one is " + cfg.in_fmt + "; Shape2D inputs move with `moving`)");
    if (o.slab_voxels && !o.moving_mesh) throw std::runtime_error("--slab-voxels: only with moving-mesh (it selects where a moving mesh is voxelised on x-slabs)");
    if (o.slab_voxels && o.nslabs < 2) throw std::runtime_error("--slab-voxels: only with GPU n for n > 1 (one GPU voxelises on the device without it)");
    if (o.slab_voxels && o.host_voxels) throw std::runtime_error("--slab-voxels: not together with --host-voxels");
    if (o.moving_mesh && o.nslabs > 1 && !o.host_voxels && !o.slab_voxels)
        throw std::runtime_error("moving-mesh: the device voxelisation runs on a single GPU only (its flood fill is global); the host voxelisation "
                                 "works on x-slabs: add --host-voxels to GPU n, or --slab-voxels (every slab voxelises and fills the whole grid on its device)");
    if ((o.time_both || o.time_geometry) && o.nslabs > 1) throw std::runtime_error("--time-both, --time-geometry: single GPU only");
    if (o.moving_mesh && o.moving) throw std::runtime_error("moving-mesh: not together with moving");
    if (o.host_voxels && !o.moving_mesh) throw std::runtime_error("--host-voxels: only with moving-mesh (it selects where a moving mesh is voxelised)");
    if (o.time_both && !o.moving_mesh) throw std::runtime_error("--time-both: only with moving-mesh (it times both ways of making a mesh's geometry)");
    if (o.time_geometry && !o.moving && !o.moving_mesh) throw std::runtime_error("--time-geometry: only with moving or moving-mesh (it times the per-step geometry work)");
    if (o.watertight && cfg.in_fmt != "Shape3D") throw std::runtime_error("--watertight: only in_fmt Shape3D inputs are meshes (this one is " + cfg.in_fmt + ")");
    if (o.wall_velocity && cfg.in_fmt != "Shape3D") throw std::runtime_error("--wall-velocity: only in_fmt Shape3D inputs are meshes (this one is " + cfg.in_fmt + ")");
    if (o.thin_shell && !o.watertight) throw std::runtime_error("--thin-shell: needs --watertight (the thin shell is a filter inside the conservative voxelisation's overlap test)");
    if (o.wall_velocity && !o.watertight) throw std::runtime_error("--wall-velocity: needs --watertight (the owner triangle of a wall cell is defined by the conservative voxelisation's overlap test)");
    if (o.has_wall_T && cfg.in_fmt != "Shape3D") throw std::runtime_error("--wall-temperature: only in_fmt Shape3D inputs are meshes (this one is " + cfg.in_fmt + ")");
    if (o.has_wall_T && !std::isfinite(o.wall_T)) throw std::runtime_error("--wall-temperature: not a finite number");
    if (o.has_wall_T && o.moving_mesh && !o.watertight) throw std::runtime_error("--wall-temperature: a moving-mesh run needs --watertight for it (the wall temperature travels with fs3d_update_nodes_shape3d_vel)");
    const bool walls = o.wall_velocity || o.has_wall_T;    // the mesh updates go through the entries that take velocities and a wall temperature
    if (walls && o.time_both) throw std::runtime_error("--time-both: not together with --wall-velocity or --wall-temperature");
    if (o.fresh_cells && !o.moving && !o.moving_mesh) throw std::runtime_error("--fresh-cells: only with moving or moving-mesh (cells turn fluid only where the geometry moves)");
    if (o.fresh_cells && o.nslabs > 1 && !o.slab_fresh_cells)
        throw std::runtime_error("--fresh-cells: single GPU only (with GPU n the fill is a collective call of all slabs: --slab-fresh-cells)");
    if (o.fresh_cells && o.time_both) throw std::runtime_error("--fresh-cells: not together with --time-both (it updates the geometry twice per step)");
    if (o.grid_time >= 0 && cfg.in_fmt != "Shape2D" && cfg.in_fmt != "Shape3D") throw std::runtime_error("--grid-time: only in_fmt Shape2D and Shape3D inputs move");
    using namespace fs3d;
    Grid3D<FTYPE> grid;
    Grid2D g2;
    Shape3D sh3;
    RunGeom geo;
    SeaNetCDF sea;
    if (cfg.in_fmt == "SeaNetCDF") {
        std::printf("Geometry: depths from NetCDF\n");                                           // FluidSolver3D.cpp:133-138
        sea.Load(grid, data, cfg.dx, cfg.dy, cfg.dz, cfg.baseT, cfg.bc_inV, cfg.bc_inT, o.align);
        geo.frames = 1; geo.length = cfg.frame_time; geo.depths = &sea.depths;                   // num_frames = 1, Grid3D.cpp:483
        for (int a = 0; a < 6; a++) geo.bbox[a] = sea.bbox[a];
    } else if (cfg.in_fmt == "Shape3D") {
        std::printf("Geometry: 3D polygons\n");                                                  // FluidSolver3D.cpp:121-126
        LoadShape3D(grid, sh3, data, cfg.dx, cfg.dy, cfg.dz, cfg.baseT, o.align, o.watertight ? 1 : 0, o.wall_velocity, o.wall_T, o.thin_shell ? 1 : 0);
        geo.frames = sh3.GetFramesNum(); geo.length = cfg.frame_time;                            // Grid3D.cpp:298-309
        for (int a = 0; a < 6; a++) geo.bbox[a] = sh3.bbox[a];
    } else {
        std::printf("Geometry: extruded 2D shape\n");                                            // :127-132
        LoadShape2D(grid, g2, data, cfg.dx, cfg.dy, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT, o.align);
        geo.frames = g2.GetFramesNum(); geo.length = g2.GetCycleLenght(); geo.g2 = &g2;
        const float bb[6] = {g2.bbox[0], g2.bbox[1], 0.0f, g2.bbox[2], g2.bbox[3], (float)cfg.depth};   // BBox3D(bbox2D, depth), :203
        for (int a = 0; a < 6; a++) geo.bbox[a] = bb[a];
    }
    std::printf("Grid = %i x %i x %i\n", grid.dimx, grid.dimy, grid.dimz);                      // FluidSolver3D.cpp:146
    double inside = 0;
    for (uint8_t t : grid.type) inside += t == NODE_IN;
    std::printf("NODE_IN points = %f of total %f, volume = %f\n", inside, (double)grid.dimx * grid.dimy * grid.dimz,
                inside * grid.dx * grid.dy * grid.dz);                                          // :170
    if (o.grid_images) OutputGridImages(grid, prefix + "_grid_3d");                             // FluidSolver3D.cpp:152-153 (there: always)
    if (!o.grid_only.empty()) {
        if (o.grid_time >= 0 && cfg.in_fmt == "Shape3D") { sh3.Prepare(o.grid_time); FillShape3DNodes(grid, sh3, cfg.baseT, o.wall_T); }
        else if (o.grid_time >= 0) { g2.Prepare(o.grid_time); ExtrudeShape2D(grid, g2, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT); }
        FILE *f = std::fopen(o.grid_only.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot create " + o.grid_only);
        const int hdr[4] = {grid.dimx, grid.dimy, grid.dimz, (int)sizeof(FTYPE)};
        std::fwrite(hdr, sizeof hdr, 1, f);
        std::fwrite(grid.type.data(), 1, grid.type.size(), f); std::fwrite(grid.bc_vel.data(), 1, grid.bc_vel.size(), f);
        std::fwrite(grid.bc_temp.data(), 1, grid.bc_temp.size(), f);
        for (const std::vector<FTYPE> *a : {&grid.vx, &grid.vy, &grid.vz, &grid.T}) std::fwrite(a->data(), sizeof(FTYPE), a->size(), f);
        std::fclose(f);
        return 0;
    }
    if (o.nslabs > 1) return run_slabs<FTYPE>(grid, g2, sh3, geo, prefix, cfg, o);
    FluidParams<FTYPE> params = cfg.useNormalizedParams ? FluidParams<FTYPE>(cfg.Re, cfg.Pr, cfg.lambda)
                                                        : FluidParams<FTYPE>(cfg.viscosity, cfg.density, cfg.R_specific, cfg.k, cfg.cv);
    AdiSolver3D<FTYPE> solver;
    solver.Init(o.device, grid, params);
    if (o.watertight) solver.SetMeshVoxels(1);           // the updates voxelise as the host loader did
    if (o.thin_shell) solver.SetMeshShell(1);
    if (o.fresh_cells) solver.SetFreshCells(true);
    if (o.output_box) solver.SetOutputFilter(1);
    if (o.time_stats) set_time_stats(solver, o);
    std::printf("Segments: %i %i %i (x, y, z)\n", solver.numSegs[0], solver.numSegs[1], solver.numSegs[2]);

    const int frames = geo.frames;                                     // FluidSolver3D.cpp:194-195
    const double length = geo.length;
    const double dt = length / (frames * cfg.time_steps);              // :196
    const double finaltime = length * cfg.cycles;
    const std::string out = prefix + "_res.nc";
    NetCDF3Writer nc;
    const float *bbox = geo.bbox;
    DepthInfo3D out_depths;                                                                  // IO.h:270-273
    if (geo.depths) out_depths = DepthInfo3D(cfg.outdimx, cfg.outdimy, *geo.depths);
    nc.Create(out, bbox, dt * cfg.out_time_steps, finaltime, cfg.outdimx, cfg.outdimy, cfg.outdimz, cfg.out_vars, geo.depths != nullptr,
              geo.depths ? out_depths.depth.data() : nullptr);
    std::vector<FTYPE> resVel((size_t)cfg.outdimx * cfg.outdimy * cfg.outdimz * 3);
    std::vector<double> resT((size_t)cfg.outdimx * cfg.outdimy * cfg.outdimz);

    solver.EnableTiming(true);
    const auto t0 = std::chrono::steady_clock::now();
    double t = dt;
    long steps = 0;
    int lastframe = -1;
    double geom_ms[3] = {0, 0, 0};                     // moving / moving-mesh: host clock around Prepare / SubFrame, the node arrays on the host, the update call
    std::vector<float> mx, my, mz;                     // moving-mesh: the sub-frame's vertices
    std::vector<float> mwx, mwy, mwz;                  // ... and their velocities (zeros without --wall-velocity)
    std::vector<double> ab_host, ab_dev, ab_dev_gpu, ab_step;   // --time-both: per step, ms
    int fill_rounds = 0;
    long long fresh_sum[2] = {0, 0}, fresh_updates = 0, fresh_rounds = 0;   // --fresh-cells: fresh and filled cells over the run, updates, most rounds of one fill
    double out_ms[2] = {0, 0};                         // --time-output: host clock around GetLayer, AppendLayer
    auto ms_since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); };
    // the geometry is frame 0's for the whole run: the reference prepares the grid once, before the loop (grid->Prepare(0), :226;
    // the per-step grid->Prepare(t) is commented out, :237) -- the frame only restarts the substep counter
    for (int i = 0; t < finaltime && (o.max_steps < 0 || steps < o.max_steps); t += dt, i++, steps++) {
        const int currentframe = geo.GetFrame(t);                                                        // :229-236
        if (currentframe != lastframe) { lastframe = currentframe; i = 0; }
        if (o.moving || o.moving_mesh) {                                                                 // grid->Prepare(t), :237
            const bool on_host = o.moving ? o.host_extrusion : o.host_voxels;     // the node arrays are made on the host and go through UpdateGrid
            if (o.time_both) {                                                                           // the other path first (mesh only)
                const auto b0 = std::chrono::steady_clock::now();
                if (o.host_voxels) { solver.UpdateGridShape3D(mx, my, mz, sh3.frames[sh3.SubFrame(t, mx, my, mz)].idx); ab_dev.push_back(ms_since(b0)); }
                else { sh3.Prepare(t); FillShape3DNodes(grid, sh3, cfg.baseT); solver.UpdateGrid(grid); ab_host.push_back(ms_since(b0)); }
            }
            const auto g0 = std::chrono::steady_clock::now();
            size_t frame = 0;
            if (o.moving) g2.Prepare(t);
            else frame = sh3.SubFrame(t, mx, my, mz);
            const auto g1 = std::chrono::steady_clock::now();
            if (on_host && o.moving) ExtrudeShape2D(grid, g2, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT);
            else if (on_host) { sh3.Prepare(t); FillShape3DNodes(grid, sh3, cfg.baseT, o.wall_T); }
            else if (o.moving_mesh && walls) {
                if (o.wall_velocity) sh3.SubFrameVelocity(t, o.wall_velocity, mwx, mwy, mwz);
                else { mwx.assign(mx.size(), 0.0f); mwy = mwx; mwz = mwx; }
            }
            const auto g3 = std::chrono::steady_clock::now();
            // (on the device, `grid` keeps the nodes of time 0: only its dims and baseT are read from here on)
            if (on_host) solver.UpdateGrid(grid);
            else if (o.moving) solver.UpdateGridExtruded(g2, cfg.dz, cfg.depth, cfg.depth_var);
            else if (walls) solver.UpdateGridShape3D(mx, my, mz, mwx, mwy, mwz, sh3.frames[frame].idx, o.wall_T);
            else solver.UpdateGridShape3D(mx, my, mz, sh3.frames[frame].idx);
            const auto g4 = std::chrono::steady_clock::now();
            if (o.fresh_cells) {                       // the cells this update turned fluid, before UpdateBoundaries
                long long info[4];
                solver.FillFreshCells(info);
                fresh_sum[0] += info[0]; fresh_sum[1] += info[1]; fresh_updates++; fresh_rounds = std::max(fresh_rounds, info[2]);
            }
            geom_ms[0] += std::chrono::duration<double, std::milli>(g1 - g0).count();
            geom_ms[1] += std::chrono::duration<double, std::milli>(g3 - g1).count();
            geom_ms[2] += std::chrono::duration<double, std::milli>(g4 - g3).count();
            if (o.time_both) (o.host_voxels ? ab_host : ab_dev).push_back(std::chrono::duration<double, std::milli>(g4 - g0).count());
        }
        if (o.time_both) {
            // (with --host-voxels the device path ran first: its device time was overwritten by the host path's update)
            float dms = 0;
            if (!o.host_voxels && fs3d_last_update_device_ms(solver.ctx(), &dms) == FS3D_OK) ab_dev_gpu.push_back(dms);
            fs3d_mesh_fill_rounds(solver.ctx(), &fill_rounds);
            fs3d_synchronize(solver.ctx());
        }
        const auto s0 = std::chrono::steady_clock::now();
        solver.UpdateBoundaries();                                                                       // :244
        solver.TimeStep((FTYPE)dt, cfg.num_global, cfg.num_local, (i % 10 == 0) || (t + dt >= finaltime)); // :245
        if (o.time_both) { fs3d_synchronize(solver.ctx()); ab_step.push_back(ms_since(s0)); }
        std::printf("\rerr = %.8f,", solver.diffError);                                                  // AdiSolver3D.cpp:376
        const float elapsed = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
        const float perres = (float)t * 100 / (float)finaltime;                                          // PrintTimeStepInfo, IO.h:455-478
        if (perres < 2) std::printf(" frame %i\tsubstep %i\t%i%%\t(----- left)", currentframe, i, (int)perres);
        else {
            const float left = elapsed * (100 - perres) / perres;
            std::printf(" frame %i\tsubstep %i\t%i%%\t(%i h %i m %i s left)", currentframe, i, (int)perres, ((int)left) / 3600, (((int)left) / 60) % 60, ((int)left) % 60);
        }
        std::fflush(stdout);
        if ((i % cfg.out_time_steps) == 0) {                                                             // :254-264
            const auto o0 = std::chrono::steady_clock::now();
            solver.GetLayer(resVel.data(), resT.data(), cfg.outdimx, cfg.outdimy, cfg.outdimz);
            const auto o1 = std::chrono::steady_clock::now();
            nc.AppendLayer(resVel.data(), resT.data());
            out_ms[0] += std::chrono::duration<double, std::milli>(o1 - o0).count(); out_ms[1] += ms_since(o1);
        }
        if (o.moving || o.moving_mesh) solver.ClearOutterCells();                                                           // AdiSolver3D.cpp:382-385
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // the reference's Profiler table (Common/Profiler.h:90-131: sorted by total time, events that never ran are absent; event
    // names of AdiSolver3D.cpp:297-367, 555-680).  Device times from HIP events; MergeLayer has no launches of its own while
    // the merge is fused into the sweep kernels; CreateSegments is the host time of the geometry upload.
    const char *names[FS3D_N_EVENTS]; float ms[FS3D_N_EVENTS]; int cnt[FS3D_N_EVENTS];
    solver.ProfilerEvents(names, ms, cnt);
    std::vector<int> order;
    for (int e = 0; e < FS3D_N_EVENTS; e++) if (cnt[e]) order.push_back(e);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return ms[a] > ms[b]; });
    double total = 0;
    if (o.csv) std::printf("\n%s,%s,%s,%s,\n", "Event Name", "Total (ms)", "Avg (ms)", "Count");
    else std::printf("\nProfiling data node(0):\n%16s%16s%16s%16s\n", "Event Name", "Total (ms)", "Avg (ms)", "Count");
    for (int e : order) {
        if (o.csv) std::printf("%s,%.2f,%.2f,%i,\n", names[e], ms[e], ms[e] / cnt[e], cnt[e]);
        else std::printf("%16s%16.2f%16.2f%16i\n", names[e], ms[e], ms[e] / cnt[e], cnt[e]);
        total += ms[e];
    }
    if (o.csv) std::printf("%s,%.2f,sec\n", "Overall", total / 1000);
    else std::printf("%16s%16.2f sec\n", "Overall", total / 1000);
    {
        int kx, ky, kz, sg;
        const char *kn[] = {"none", "line", "pipe", "part"};
        fs3d_last_sweep_kernel(solver.ctx(), 0, &kx, &sg); fs3d_last_sweep_kernel(solver.ctx(), 1, &ky, &sg); fs3d_last_sweep_kernel(solver.ctx(), 2, &kz, &sg);
        std::printf("Sweep kernels: X %s, Y %s, Z %s\n", kn[kx & 3], kn[ky & 3], kn[kz & 3]);
    }
    if (o.fresh_cells) std::printf("Fresh cells: %lld in %lld updates, %lld filled, at most %lld rounds\n", fresh_sum[0], fresh_updates, fresh_sum[1], fresh_rounds);
    if (o.time_geometry && steps > 0)                  // (before the line of --time-both, which only a mesh has)
        std::printf(o.moving ? "Moving geometry per step (host clock, ms): Prepare %.3f, extrusion on the host %.3f, update call %.3f; step %.3f\n"
                             : "Moving mesh per step (host clock, ms): SubFrame %.3f, voxels on the host %.3f, update call %.3f; step %.3f\n",
                    geom_ms[0] / steps, geom_ms[1] / steps, geom_ms[2] / steps, sec * 1e3 / steps);
    if (o.time_both) {
        auto line = [](const char *what, std::vector<double> v) {
            if (v.size() <= 3) { std::printf(" %s: too few steps;", what); return; }
            v.erase(v.begin(), v.begin() + 3);
            std::sort(v.begin(), v.end());
            const size_t n = v.size();
            std::printf(" %s median %.3f min %.3f max %.3f n %zu;", what, n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]), v.front(), v.back(), n);
        };
        std::printf("Moving mesh, both paths per call (ms):");
        line("host voxels + fs3d_update_nodes", ab_host); line("fs3d_update_nodes_shape3d", ab_dev); line("its device time", ab_dev_gpu);
        line("time step", ab_step);
        std::printf(" fill rounds %d\n", fill_rounds);
    }
    if (o.time_output && nc.NumRecords() > 0)
        std::printf("Result output per record (host clock, ms): GetLayer %.3f, AppendLayer %.3f; %u records\n", out_ms[0] / nc.NumRecords(),
                    out_ms[1] / nc.NumRecords(), nc.NumRecords());
    std::printf("%ld steps in %.3f s: %.1f Mcells/s; %u layers in %s\n", steps, sec,
                (double)grid.dimx * grid.dimy * grid.dimz * steps / sec / 1e6, nc.NumRecords(), out.c_str());
    if (o.time_stats) {
        const std::string stats = prefix + "_stats.nc";
        if (steps > 0) {
            NetCDF3Writer ns;
            ns.Create(stats, bbox, dt * cfg.out_time_steps, finaltime, cfg.outdimx, cfg.outdimy, cfg.outdimz, cfg.out_vars, geo.depths != nullptr,
                      geo.depths ? out_depths.depth.data() : nullptr);
            for (const StatsRecord &rec : stats_records(o)) {
                solver.SetOutputSource(rec.source);
                if (o.time_cov) solver.SetOutputMoment(rec.moment);
                solver.GetLayer(resVel.data(), resT.data(), cfg.outdimx, cfg.outdimy, cfg.outdimz);
                ns.AppendLayer(resVel.data(), resT.data());
            }
            solver.SetOutputSource(0);
        }
        print_stats_line(steps, o, stats);
    }
    return 0;
}

// "GPU n" with n > 1: the reference's single-process multi-GPU mode (GPUplan): n x-slabs (GPUplan::splitEven1D,
// GPUplan.cpp:122-141), one solver and one host thread per slab, joined by the library's in-process group.
// Results equal the single-GPU run's value for value.  Slab r runs on device r, or all on device 0 with --same-device.
// moving / moving-mesh --host-voxels: rank 0 prepares the geometry of time t on the host (Prepare, and the host extrusion or
// voxelisation into the shared Grid3D where asked), a barrier, then every rank rebuilds the tables of its own planes from that
// global input (UpdateGrid / UpdateGridExtruded: the slab entries, no rank waits for another inside them).
// moving-mesh --slab-voxels: rank 0 computes the sub-frame's vertices (and their velocities) into shared vectors, a barrier, then
// every rank voxelises the mesh for itself (UpdateGridShape3D: the slab entries).  Either way, after the step
// ClearOutterCells on every rank, and a barrier before rank 0 prepares the next geometry in the arrays the others have read.
namespace {
struct Barrier {
    std::mutex m; std::condition_variable cv; int n, waiting = 0; long gen = 0; bool broken = false;
    explicit Barrier(int n_) : n(n_) {}
    void wait()
    {
        std::unique_lock<std::mutex> lk(m);
        const long g = gen;
        if (++waiting == n) { waiting = 0; gen++; cv.notify_all(); } else cv.wait(lk, [&] { return gen != g || broken; });
        if (broken) throw std::runtime_error("another slab thread failed");
    }
    void abort() { { std::lock_guard<std::mutex> lk(m); broken = true; } cv.notify_all(); }
};
}

template <typename FTYPE>
static int run_slabs(fs3d::Grid3D<FTYPE> &grid, fs3d::Grid2D &g2, fs3d::Shape3D &sh3, const RunGeom &geo, const std::string &prefix,
                     const fs3d::Config &cfg, const RunOptions &o)
{
    using namespace fs3d;
    const int nslabs = o.nslabs;
    const bool same_device = o.same_device, time_output = o.time_output, moves = o.moving || o.moving_mesh;
    const bool on_host = o.moving ? o.host_extrusion : o.host_voxels;
    const bool walls = o.wall_velocity || o.has_wall_T;    // --slab-voxels: the entry that takes velocities and a wall temperature
    std::vector<float> mx, my, mz, mwx, mwy, mwz;          // --slab-voxels: the sub-frame of the step, written by rank 0 and read by all
    size_t mframe = 0;
    const long max_steps = o.max_steps;
    // --slab-fresh-cells: every rank's own fresh and filled cells over the run; the updates and the most rounds of one fill (the group's: rank 0 writes them)
    std::vector<long long> fresh_own(nslabs, 0), filled_own(nslabs, 0);
    long long fresh_updates = 0, fresh_rounds = 0;
    FluidParams<FTYPE> params = cfg.useNormalizedParams ? FluidParams<FTYPE>(cfg.Re, cfg.Pr, cfg.lambda)
                                                        : FluidParams<FTYPE>(cfg.viscosity, cfg.density, cfg.R_specific, cfg.k, cfg.cv);
    const double length = geo.length, dt = length / (geo.frames * cfg.time_steps), finaltime = length * cfg.cycles;
    const std::string out = prefix + "_res.nc";
    NetCDF3Writer nc, ns;                              // ns: --time-stats, <prefix>_stats.nc (rank 0 creates and appends)
    const std::string stats = prefix + "_stats.nc";
    const float *bbox = geo.bbox;
    DepthInfo3D out_depths;                                                                  // IO.h:270-273
    if (geo.depths) out_depths = DepthInfo3D(cfg.outdimx, cfg.outdimy, *geo.depths);
    nc.Create(out, bbox, dt * cfg.out_time_steps, finaltime, cfg.outdimx, cfg.outdimy, cfg.outdimz, cfg.out_vars, geo.depths != nullptr,
              geo.depths ? out_depths.depth.data() : nullptr);
    std::vector<FTYPE> resVel((size_t)cfg.outdimx * cfg.outdimy * cfg.outdimz * 3);
    std::vector<double> resT((size_t)cfg.outdimx * cfg.outdimy * cfg.outdimz);
    double out_ms[2] = {0, 0};                         // --time-output (rank 0): host clock until the record is complete, AppendLayer
    void *group = AdiSolver3D<FTYPE>::CreateLocalGroup(nslabs);
    Barrier bar(nslabs);
    std::vector<std::exception_ptr> errs(nslabs);
    std::vector<std::thread> th;
    long steps_done = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < nslabs; r++)
        th.emplace_back([&, r] {
            try {
                const int q = grid.dimx / nslabs, rem = grid.dimx % nslabs;
                const int x0 = r * q + std::min(r, rem), x1 = x0 + q + (r < rem ? 1 : 0);
                AdiSolver3D<FTYPE> solver;
                solver.Init(same_device ? 0 : r, grid, params, x0, x1);
                solver.JoinLocalGroup(group, r);
                if (o.watertight) solver.SetMeshVoxels(1);           // the updates voxelise as the host loader did
                if (o.thin_shell) solver.SetMeshShell(1);
                if (o.fresh_cells) { solver.SetFreshCells(true); solver.SetFreshCellsSlabs(true); }
                if (o.time_stats) set_time_stats(solver, o);
                // every rank has uploaded the grid of time 0 before rank 0 writes the next geometry into the same arrays (Init
                // reads them, and joining the group is no rendezvous)
                if (moves) bar.wait();
                if (r == 0) std::printf("Slabs: %d x-slabs of %d..%d planes\n", nslabs, q, q + (rem ? 1 : 0));
                double t = dt;
                long steps = 0;
                int lastframe = -1;
                for (int i = 0; t < finaltime && (max_steps < 0 || steps < max_steps); t += dt, i++, steps++) {
                    const int currentframe = geo.GetFrame(t);
                    if (currentframe != lastframe) { lastframe = currentframe; i = 0; }
                    if (moves) {
                        if (r == 0) {
                            if (o.moving) { g2.Prepare(t); if (on_host) ExtrudeShape2D(grid, g2, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT); }
                            else if (on_host) { sh3.Prepare(t); FillShape3DNodes(grid, sh3, cfg.baseT, o.wall_T); }
                            else {
                                mframe = sh3.SubFrame(t, mx, my, mz);
                                if (o.wall_velocity) sh3.SubFrameVelocity(t, o.wall_velocity, mwx, mwy, mwz);
                                else if (walls) { mwx.assign(mx.size(), 0.0f); mwy = mwx; mwz = mwx; }
                            }
                        }
                        bar.wait();
                        if (on_host) solver.UpdateGrid(grid);
                        else if (o.moving) solver.UpdateGridExtruded(g2, cfg.dz, cfg.depth, cfg.depth_var);
                        else if (walls) solver.UpdateGridShape3D(mx, my, mz, mwx, mwy, mwz, sh3.frames[mframe].idx, o.wall_T);
                        else solver.UpdateGridShape3D(mx, my, mz, sh3.frames[mframe].idx);
                        if (o.fresh_cells) {               // the cells this update turned fluid, all slabs together, before UpdateBoundaries
                            long long info[4];
                            solver.FillFreshCells(info);
                            fresh_own[r] += info[0]; filled_own[r] += info[1];
                            if (r == 0) { fresh_updates++; fresh_rounds = std::max(fresh_rounds, info[2]); }
                        }
                    }
                    solver.UpdateBoundaries();
                    solver.TimeStep((FTYPE)dt, cfg.num_global, cfg.num_local, (i % 10 == 0) || (t + dt >= finaltime));
                    if (r == 0) { std::printf("\rerr = %.8f, frame %i\tsubstep %i\t%i%%", solver.diffError, currentframe, i, (int)((float)t * 100 / (float)finaltime)); std::fflush(stdout); }
                    if ((i % cfg.out_time_steps) == 0) {
                        // each slab samples the rows of the result whose source planes it owns (FilterToArrays, TimeLayer3D.h:819-924)
                        // straight into the shared arrays: the rows are disjoint
                        const auto o0 = std::chrono::steady_clock::now();
                        int rows[2];
                        solver.GetLayerRows(resVel.data(), resT.data(), cfg.outdimx, cfg.outdimy, cfg.outdimz, rows);
                        bar.wait();
                        if (r == 0) {
                            const auto o1 = std::chrono::steady_clock::now();
                            nc.AppendLayer(resVel.data(), resT.data());
                            out_ms[0] += std::chrono::duration<double, std::milli>(o1 - o0).count();
                            out_ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - o1).count();
                        }
                        bar.wait();                    // nobody writes the next record's rows while rank 0 still reads this one
                    }
                    if (moves) { solver.ClearOutterCells(); bar.wait(); }      // AdiSolver3D.cpp:382-385; every rank has read this step's geometry
                }
                if (r == 0) steps_done = steps;
                if (o.time_stats && steps > 0) {
                    // the statistics records as the normal ones: every slab writes its rows of the shared arrays, rank 0 appends
                    if (r == 0) ns.Create(stats, bbox, dt * cfg.out_time_steps, finaltime, cfg.outdimx, cfg.outdimy, cfg.outdimz, cfg.out_vars,
                                          geo.depths != nullptr, geo.depths ? out_depths.depth.data() : nullptr);
                    for (const StatsRecord &rec : stats_records(o)) {
                        int rows[2];
                        solver.SetOutputSource(rec.source);
                        if (o.time_cov) solver.SetOutputMoment(rec.moment);
                        solver.GetLayerRows(resVel.data(), resT.data(), cfg.outdimx, cfg.outdimy, cfg.outdimz, rows);
                        bar.wait();
                        if (r == 0) ns.AppendLayer(resVel.data(), resT.data());
                        bar.wait();
                    }
                    solver.SetOutputSource(0);
                }
            } catch (...) {
                // release the other slab threads: they wait for this one in the transport (halo planes, carries) or at the
                // output barrier and would never return
                errs[r] = std::current_exception();
                fs3d_local_group_abort(group);
                bar.abort();
            }
        });
    for (auto &t : th) t.join();
    AdiSolver3D<FTYPE>::DestroyLocalGroup(group);
    for (auto &e : errs) if (e) {          // the first failure, not the "another slab thread failed" it caused
        try { std::rethrow_exception(e); } catch (std::exception &x) { if (std::string(x.what()).find("another slab thread") == std::string::npos && std::string(x.what()).find("a peer failed") == std::string::npos) throw; } catch (...) { throw; }
    }
    for (auto &e : errs) if (e) std::rethrow_exception(e);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("\n");
    if (o.fresh_cells) {
        long long fresh = 0, filled = 0;
        for (int r = 0; r < nslabs; r++) { fresh += fresh_own[r]; filled += filled_own[r]; }
        std::printf("Fresh cells: %lld in %lld updates, %lld filled, at most %lld rounds\n", fresh, fresh_updates, filled, fresh_rounds);
    }
    if (time_output && nc.NumRecords() > 0)
        std::printf("Result output per record (host clock, ms): GetLayer %.3f, AppendLayer %.3f; %u records\n", out_ms[0] / nc.NumRecords(),
                    out_ms[1] / nc.NumRecords(), nc.NumRecords());
    std::printf("%ld steps in %.3f s: %.1f Mcells/s; %u layers in %s\n", steps_done, sec,
                (double)grid.dimx * grid.dimy * grid.dimz * steps_done / sec / 1e6, nc.NumRecords(), out.c_str());
    if (o.time_stats) print_stats_line(steps_done, o, stats);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::printf("Usage: %s <input data> <output prefix> <config file> [align] [GPU [n]] [double] [--steps N] [moving [--host-extrusion] [--time-geometry]] [moving-mesh [--host-voxels | --slab-voxels] [--time-geometry] [--time-both]] [--time-output] [--grid-only FILE [--grid-time T]] [--grid-images] [--watertight [--thin-shell] [--wall-velocity motion|file]] [--wall-temperature T] [--fresh-cells | --slab-fresh-cells] [--output-filter point|box] [--time-stats mean|variance] [--time-covariances] [--time-stats-every K]\n", argv[0]);
        return 0;
    }
    try {
        fs3d::Config cfg;
        cfg.Load(argv[3]);
        if (cfg.problem_dim != "3D") throw std::runtime_error("only `dimension 3D` runs are supported");
        if (cfg.in_fmt != "Shape2D" && cfg.in_fmt != "Shape3D" && cfg.in_fmt != "SeaNetCDF") throw std::runtime_error("in_fmt " + cfg.in_fmt + ": unknown input format");
        if (cfg.in_fmt != "Shape2D" && !(cfg.frame_time > 0)) throw std::runtime_error("must specify frame time!");   // the cycle length of a Shape3D run (Grid3D.cpp:303-309)
        if (cfg.solver != "ADI") throw std::runtime_error("solver " + cfg.solver + " is not implemented (the reference implements ADI only)");
        RunOptions o;
        for (int a = 4; a < argc; a++) {
            const std::string s = argv[a];
            if (s == "align") o.align = true;
            else if (s == "GPU") { if (a + 1 < argc && std::atoi(argv[a + 1]) > 0) o.nslabs = std::atoi(argv[++a]); }   // the reference's "GPU n": n devices of one process
            else if (s == "--same-device") o.same_device = true;
            else if (s == "double") o.dbl = true;
            else if (s == "--device" && a + 1 < argc) o.device = std::atoi(argv[++a]);
            else if (s == "--steps" && a + 1 < argc) o.max_steps = std::atol(argv[++a]);
            else if (s == "--grid-only" && a + 1 < argc) o.grid_only = argv[++a];
            else if (s == "--grid-time" && a + 1 < argc) o.grid_time = std::atof(argv[++a]);
            else if (s == "moving") o.moving = true;
            else if (s == "moving-mesh") o.moving_mesh = true;
            else if (s == "--host-voxels") o.host_voxels = true;
            else if (s == "--slab-voxels") o.slab_voxels = true;
            else if (s == "--watertight") o.watertight = true;
            else if (s == "--thin-shell") o.thin_shell = true;
            else if (s == "--wall-velocity") {
                const std::string w = a + 1 < argc ? argv[++a] : "";
                if (w != "motion" && w != "file") throw std::runtime_error("--wall-velocity: motion or file");
                o.wall_velocity = w == "motion" ? 1 : 2;
            }
            else if (s == "--wall-temperature") {
                if (a + 1 >= argc) throw std::runtime_error("--wall-temperature: a number follows");
                char *end = nullptr;
                o.wall_T = std::strtod(argv[++a], &end); o.has_wall_T = true;
                if (end == argv[a] || *end) throw std::runtime_error("--wall-temperature: not a number");
            }
            else if (s == "--fresh-cells") o.fresh_cells = true;
            else if (s == "--slab-fresh-cells") o.fresh_cells = o.slab_fresh_cells = true;
            else if (s == "--output-filter") {
                const std::string w = a + 1 < argc ? argv[++a] : "";
                if (w != "point" && w != "box") throw std::runtime_error("--output-filter: point or box");
                o.output_box = w == "box";
            }
            else if (s == "--time-stats") {
                const std::string w = a + 1 < argc ? argv[++a] : "";
                if (w != "mean" && w != "variance") throw std::runtime_error("--time-stats: mean or variance");
                o.time_stats = w == "mean" ? 1 : 2;
            }
            else if (s == "--time-covariances") o.time_cov = true;
            else if (s == "--time-stats-every") {
                const char *const w = a + 1 < argc ? argv[++a] : "";
                char *end = nullptr;
                o.time_every = std::strtol(w, &end, 10);
                if (end == w || *end || o.time_every < 1 || o.time_every > (1L << 20))
                    throw std::runtime_error("--time-stats-every: an integer from 1 to 1048576 follows");
            }
            else if (s == "--time-both") o.time_both = true;
            else if (s == "--host-extrusion") o.host_extrusion = true;
            else if (s == "--time-geometry") o.time_geometry = true;
            else if (s == "--time-output") o.time_output = true;
            else if (s == "blocking") { if (a + 1 < argc) a++; }
            else if (s == "CSV") o.csv = true;
            else if (s == "--grid-images") o.grid_images = true;       // <prefix>_grid_3d/<k>.bmp: the node types, one image per z-slice
            // transpose, decompose: accepted, no effect
        }
        if (o.time_cov && o.time_stats != 2) throw std::runtime_error("--time-covariances: needs --time-stats variance");
        if (o.output_box && o.nslabs > 1)
            throw std::runtime_error("--output-filter box: single GPU only (with GPU n the grid is cut into x-slabs, a sample's box of source cells can "
                                     "straddle a cut, and the library refuses filtered records on a slab)");
        return o.dbl ? run<double>(argv[1], argv[2], cfg, o) : run<float>(argv[1], argv[2], cfg, o);
    } catch (std::exception &e) {
        std::fprintf(stderr, "\n\nCaught exception:\n%s\n\nTerminating...\n", e.what());     // FluidSolver3D.cpp:313-318
        return -1;
    }
}
