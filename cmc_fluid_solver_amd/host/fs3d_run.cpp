// Command-line driver: the reference's FluidSolver3D main (FluidSolver3D/FluidSolver3D.cpp:60-330) on top of
// libfs3d_hip.so.   fs3d_run <input data> <output prefix> <config file> [words]: the words are those of USAGE below, which main prints.
//   * reads the config (host/Config.h) and a Shape2D, Shape3D or SeaNetCDF geometry (host/Shape2D.h, Shape3D.h, SeaNetCDF.h), prints the grid summary lines
//     the reference prints ("Grid = X x Y x Z", "NODE_IN points = ..."),
//   * runs the same loop, ONE loop for a single GPU and for `GPU n` (run_loop below: the single GPU is its one-rank case): dt = cycle length /
//     (frames * time_steps), UpdateBoundaries + TimeStep per step with the
//     divergence error every 10th step and on the last one, "err = ..." and the progress line per step,
//   * writes <output prefix>_res.nc through host/NetCDF3.h every out_time_steps steps (GetLayer).
// `transpose`, `decompose`, `blocking n` of the reference are accepted and ignored (backend tuning switches); `CSV`
// switches the closing timing table to the reference's comma-separated form.
// `moving` (in_fmt Shape2D; one GPU, or GPU n --same-device): the walls follow the frames of the input -- per step grid2D->Prepare(t), the extrusion and
//   CreateSegments on the device (UpdateGridExtruded: the 2D grid travels, the node arrays are written by a kernel), UpdateBoundaries,
//   TimeStep, the output, ClearOutterCells: the loop of the reference's 2D driver (FluidSolver2D.cpp:130-133) with the 3D classes'
//   mechanism (AdiSolver3D.cpp:382-385, Solver3D.cpp:41-44).
//   --host-extrusion: the extrusion on the host (ExtrudeShape2D into the Grid3D, then UpdateGrid with its seven arrays) -- the same
//   results bit for bit; kept for A/B timing and as the checker of the device extrusion.
//   --time-geometry: one more line after the timing table, the host clock per step around Prepare, the host extrusion and the update call.
// `moving-mesh` (in_fmt Shape3D; one GPU, or GPU n with --host-voxels or --slab-voxels): the same loop for a triangle mesh per frame -- per step Shape3D::SubFrame(t) (the
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
// --slab-output-filter point|box: --output-filter that also runs with GPU n -- `box` calls SetOutputSlabs(1) and SetOutputFilter(1) on every
//   slab before the loop (FS3D_OPT_OUTPUT_SLABS): every record, the ones of <prefix>_stats.nc among them, is then a collective call of
//   the slabs, which add the partial sums of the rows whose box straddles a cut, and holds the global grid's box means.  With an
//   output grid at least as fine as the grid the file is the single-GPU run's, byte for byte.  With one GPU it is --output-filter.
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
// --time-gradients, with --time-stats (else refused when the arguments are read; refused with GPU n, n > 1, too): SetTimeStatsGradients(1)
//   before the loop -- every accumulated step also adds the invariants of its velocity gradient, div u, Q and S:S, to per-cell sums
//   (FS3D_OPT_TIME_STATS_GRAD) -- and <prefix>_stats.nc holds one more record, directly before the fluid fraction, which stays last: the
//   time mean of div u in u, of Q in v, of S:S in w and of T in T (source 1 with SetOutputGradient(2)).  The closing line gains
//   `, gradients`.  Without the word every file and every print is unchanged.
// --time-wall, with --time-stats (else refused when the arguments are read; refused with GPU n, n > 1, too): SetTimeStatsWall(1) before
//   the loop -- every accumulated step also adds the wall shear stress, its magnitude and the wall heat flux to per-cell sums on the
//   wall cells that carry them (FS3D_OPT_TIME_STATS_WALL) -- and <prefix>_stats.nc holds two more records, directly before the fluid
//   fraction, which stays last, and after the record of --time-gradients: the time mean of the wall shear stress vector in u, v, w
//   (source 1 with SetOutputWall(3)), then the time-averaged magnitude (TAWSS) in u, the mean wall heat flux in v and the oscillatory
//   shear index in w (SetOutputWall(4)); T is the mean of T in both.  --output-filter box applies to them (the mean over the wall
//   cells under a sample).  The closing line gains `, wall`.  Without the word every file and every print is unchanged.
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
    bool has_wall_T = false, fresh_cells = false, slab_fresh_cells = false, output_box = false, slab_output_box = false;
    int time_stats = 0;                                // --time-stats: 0 none, 1 mean, 2 mean and variance (FS3D_OPT_TIME_STATS)
    bool time_cov = false;                             // --time-covariances (FS3D_OPT_TIME_STATS_CROSS; needs time_stats 2)
    long time_every = 1;                               // --time-stats-every K (FS3D_OPT_TIME_STATS_EVERY)
    bool time_grad = false;                            // --time-gradients (FS3D_OPT_TIME_STATS_GRAD; needs time_stats, one GPU)
    bool time_wall = false;                            // --time-wall (FS3D_OPT_TIME_STATS_WALL; needs time_stats, one GPU)
    int nslabs = 1, device = 0;
    long max_steps = -1;
    std::string grid_only;
    bool moves() const { return moving || moving_mesh; }
    bool on_host() const { return moving ? host_extrusion : host_voxels; }   // the node arrays are made on the host and go through UpdateGrid
    bool walls() const { return wall_velocity || has_wall_T; }               // the mesh updates go through the entries that take velocities and a wall temperature
};

static const char USAGE[] = "<input data> <output prefix> <config file> [align] [GPU [n]] [double] [--steps N] [moving [--host-extrusion] [--time-geometry]] [moving-mesh [--host-voxels | --slab-voxels] [--time-geometry] [--time-both]] [--time-output] [--grid-only FILE [--grid-time T]] [--grid-images] [--watertight [--thin-shell] [--wall-velocity motion|file]] [--wall-temperature T] [--fresh-cells | --slab-fresh-cells] [--output-filter point|box] [--slab-output-filter point|box] [--time-stats mean|variance] [--time-covariances] [--time-stats-every K] [--time-gradients] [--time-wall]";

// the refusals that need no geometry, in the order a user meets them
static void check_words(const RunOptions &o, const fs3d::Config &cfg)
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
    if (o.walls() && o.time_both) throw std::runtime_error("--time-both: not together with --wall-velocity or --wall-temperature");
    if (o.fresh_cells && !o.moving && !o.moving_mesh) throw std::runtime_error("--fresh-cells: only with moving or moving-mesh (cells turn fluid only where the geometry moves)");
    if (o.fresh_cells && o.nslabs > 1 && !o.slab_fresh_cells)
        throw std::runtime_error("--fresh-cells: single GPU only (with GPU n the fill is a collective call of all slabs: --slab-fresh-cells)");
    if (o.fresh_cells && o.time_both) throw std::runtime_error("--fresh-cells: not together with --time-both (it updates the geometry twice per step)");
    if (o.grid_time >= 0 && cfg.in_fmt != "Shape2D" && cfg.in_fmt != "Shape3D") throw std::runtime_error("--grid-time: only in_fmt Shape2D and Shape3D inputs move");
}

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// --time-stats: the records of <prefix>_stats.nc, in order, each a source and a moment (FS3D_OPT_OUTPUT_SOURCE: 1 mean, 2 second
// moments, 3 fluid fraction; FS3D_OPT_OUTPUT_MOMENT: 0 variance, 1 stresses, 2 heat flux)
// --time-gradients: one more record directly before the fluid fraction, source 1 with FS3D_OPT_OUTPUT_GRADIENT 2
// --time-wall: two more behind it, source 1 with FS3D_OPT_OUTPUT_WALL 3 and 4
struct StatsRecord { int source, moment, gradient, wall; };
static std::vector<StatsRecord> stats_records(const RunOptions &o)
{
    std::vector<StatsRecord> recs = {{1, 0, 0, 0}};
    if (o.time_stats == 2) recs.push_back({2, 0, 0, 0});
    if (o.time_stats == 2 && o.time_cov) { recs.push_back({2, 1, 0, 0}); recs.push_back({2, 2, 0, 0}); }
    if (o.time_grad) recs.push_back({1, 0, 2, 0});
    if (o.time_wall) { recs.push_back({1, 0, 0, 3}); recs.push_back({1, 0, 0, 4}); }
    recs.push_back({3, 0, 0, 0});
    return recs;
}

// what a solver is told before the loop; nslabs > 1: it is a slab of a group
template <class Solver>
static void apply_options(Solver &solver, const RunOptions &o, int nslabs)
{
    if (o.watertight) solver.SetMeshVoxels(1);           // the updates voxelise as the host loader did
    if (o.thin_shell) solver.SetMeshShell(1);
    if (o.fresh_cells) solver.SetFreshCells(true);
    if (o.fresh_cells && nslabs > 1) solver.SetFreshCellsSlabs(true);
    if (o.output_box && nslabs > 1) solver.SetOutputSlabs(1);   // --slab-output-filter box (check in main: the plain word never gets here with slabs)
    if (o.output_box) solver.SetOutputFilter(1);
    if (o.time_stats) solver.SetTimeStats(o.time_stats);
    if (o.time_stats && o.time_cov) solver.SetTimeStatsCross(1);
    if (o.time_stats && o.time_every > 1) solver.SetTimeStatsEvery((int)o.time_every);
    if (o.time_stats && o.time_grad) solver.SetTimeStatsGradients(1);
    if (o.time_stats && o.time_wall) solver.SetTimeStatsWall(1);
}

// The ranks wait for one another here.  One rank: every wait returns at once.
namespace {
struct Barrier {
    std::mutex m; std::condition_variable cv; int n, waiting = 0; long gen = 0; bool broken = false;
    explicit Barrier(int n_) : n(n_) {}
    void wait()
    {
        std::unique_lock<std::mutex> lk(m);
        const long g = gen;
        if (++waiting == n) { waiting = 0; gen++; cv.notify_all(); return; }
        cv.wait(lk, [&] { return gen != g || broken; });
        // a rank that every other rank has joined here goes on, whatever has failed since: how far the ranks get beside a failing one
        // does not depend on which of them wakes first
        if (gen == g) throw std::runtime_error("another slab thread failed");
    }
    void abort() { { std::lock_guard<std::mutex> lk(m); broken = true; } cv.notify_all(); }
};
}

// What the ranks of a run share.  A single GPU is the run of one rank; "GPU n" with n > 1 is the reference's single-process
// multi-GPU mode (GPUplan): n x-slabs (GPUplan::splitEven1D, GPUplan.cpp:122-141), one solver and one host thread per slab,
// joined by the library's in-process group; its results equal the single-GPU run's value for value.  Slab r runs on device r, or
// all on device 0 with --same-device.  Rank 0 alone writes the grid, the 2D grid, the sub-frame vectors, both files and the
// counters that are no per-rank vector; the barrier says when the others may read them.
template <typename FTYPE>
struct Run {
    fs3d::Grid3D<FTYPE> &grid; fs3d::Grid2D &g2; fs3d::Shape3D &sh3;
    const RunGeom &geo; const fs3d::Config &cfg; const RunOptions &o;
    const int nslabs;
    const fs3d::FluidParams<FTYPE> params;
    const double dt, finaltime;                        // FluidSolver3D.cpp:194-196
    const std::string out, stats;
    fs3d::NetCDF3Writer nc, ns;                        // <prefix>_res.nc; --time-stats: <prefix>_stats.nc
    fs3d::DepthInfo3D out_depths;                      // IO.h:270-273
    std::vector<FTYPE> resVel;                         // one record: every rank writes the rows it owns, rank 0 appends
    std::vector<double> resT;
    Barrier bar;
    void *group = nullptr;
    std::vector<float> mx, my, mz, mwx, mwy, mwz;      // moving-mesh on the device: the sub-frame's vertices and their velocities (zeros without --wall-velocity)
    size_t mframe = 0;
    std::vector<long long> fresh_own, filled_own;      // --fresh-cells: every rank's own fresh and filled cells over the run
    long long fresh_updates = 0, fresh_rounds = 0;     // ... the updates and the most rounds of one fill (the group's)
    double out_ms[2] = {0, 0};                         // --time-output: host clock until the record is complete, AppendLayer
    Clock::time_point t0;
    long steps = 0;
    double sec = 0;
    // the single-GPU measurement words
    double geom_ms[3] = {0, 0, 0};                     // --time-geometry: host clock around Prepare / SubFrame, the node arrays on the host, the update call
    std::vector<double> ab_host, ab_dev, ab_dev_gpu, ab_step;   // --time-both: per step, ms
    int fill_rounds = 0;

    Run(fs3d::Grid3D<FTYPE> &grid_, fs3d::Grid2D &g2_, fs3d::Shape3D &sh3_, const RunGeom &geo_, const std::string &prefix,
        const fs3d::Config &cfg_, const RunOptions &o_)
        : grid(grid_), g2(g2_), sh3(sh3_), geo(geo_), cfg(cfg_), o(o_), nslabs(o_.nslabs),
          params(cfg_.useNormalizedParams ? fs3d::FluidParams<FTYPE>(cfg_.Re, cfg_.Pr, cfg_.lambda)
                                          : fs3d::FluidParams<FTYPE>(cfg_.viscosity, cfg_.density, cfg_.R_specific, cfg_.k, cfg_.cv)),
          dt(geo_.length / (geo_.frames * cfg_.time_steps)), finaltime(geo_.length * cfg_.cycles),
          out(prefix + "_res.nc"), stats(prefix + "_stats.nc"),
          resVel((size_t)cfg_.outdimx * cfg_.outdimy * cfg_.outdimz * 3), resT((size_t)cfg_.outdimx * cfg_.outdimy * cfg_.outdimz),
          bar(o_.nslabs), fresh_own(o_.nslabs, 0), filled_own(o_.nslabs, 0)
    {
        if (geo.depths) out_depths = fs3d::DepthInfo3D(cfg.outdimx, cfg.outdimy, *geo.depths);
    }
    void create_result_file(fs3d::NetCDF3Writer &file, const std::string &name)
    {
        file.Create(name, geo.bbox, dt * cfg.out_time_steps, finaltime, cfg.outdimx, cfg.outdimy, cfg.outdimz, cfg.out_vars, geo.depths != nullptr,
                    geo.depths ? out_depths.depth.data() : nullptr);
    }
};

// The geometry of time t, first half: what rank 0 does on the host.  on_host: the node arrays are made here, in the shared grid
// (--host-extrusion, --host-voxels); else the 2D grid of time t, or the sub-frame's vertices and their velocities, are what travels.
// *mid: the clock between Prepare / SubFrame and the rest (--time-geometry).
// (on the device, `grid` keeps the nodes of time 0: only its dims and baseT are read from here on)
template <typename FTYPE>
static void prepare_geometry(Run<FTYPE> &s, double t, bool on_host, Clock::time_point *mid = nullptr)
{
    const RunOptions &o = s.o;
    const fs3d::Config &cfg = s.cfg;
    if (o.moving) s.g2.Prepare(t);                                                                   // grid->Prepare(t), FluidSolver3D.cpp:237
    else if (!on_host) s.mframe = s.sh3.SubFrame(t, s.mx, s.my, s.mz);
    if (mid) *mid = Clock::now();
    if (on_host && o.moving) ExtrudeShape2D(s.grid, s.g2, cfg.dz, cfg.depth, cfg.depth_var, cfg.baseT);
    else if (on_host) { s.sh3.Prepare(t); FillShape3DNodes(s.grid, s.sh3, cfg.baseT, o.wall_T); }
    else if (o.wall_velocity) s.sh3.SubFrameVelocity(t, o.wall_velocity, s.mwx, s.mwy, s.mwz);
    else if (o.walls()) { s.mwx.assign(s.mx.size(), 0.0f); s.mwy = s.mwx; s.mwz = s.mwx; }
}
// ... second half: what every rank then asks of its solver, which rebuilds the tables of its own planes from that global input
// (the slab entries on a slab: no rank waits for another inside them)
template <typename FTYPE>
static void update_geometry(Run<FTYPE> &s, fs3d::AdiSolver3D<FTYPE> &solver, bool on_host)
{
    const RunOptions &o = s.o;
    if (on_host) solver.UpdateGrid(s.grid);
    else if (o.moving) solver.UpdateGridExtruded(s.g2, s.cfg.dz, s.cfg.depth, s.cfg.depth_var);
    else if (o.walls()) solver.UpdateGridShape3D(s.mx, s.my, s.mz, s.mwx, s.mwy, s.mwz, s.sh3.frames[s.mframe].idx, o.wall_T);
    else solver.UpdateGridShape3D(s.mx, s.my, s.mz, s.sh3.frames[s.mframe].idx);
}

// One record into `file`.  One rank: GetLayer.  Several: each slab samples the rows of the result whose source planes it owns
// (FilterToArrays, TimeLayer3D.h:819-924) straight into the shared arrays -- the rows are disjoint -- and rank 0 appends once every
// rank has written its rows.  ms (--time-output, may be NULL): rank 0's host clock until the record is complete, and around AppendLayer.
template <typename FTYPE>
static void record(Run<FTYPE> &s, fs3d::AdiSolver3D<FTYPE> &solver, int r, fs3d::NetCDF3Writer &file, double *ms)
{
    const auto o0 = Clock::now();
    int rows[2];
    if (s.nslabs == 1) solver.GetLayer(s.resVel.data(), s.resT.data(), s.cfg.outdimx, s.cfg.outdimy, s.cfg.outdimz);
    else solver.GetLayerRows(s.resVel.data(), s.resT.data(), s.cfg.outdimx, s.cfg.outdimy, s.cfg.outdimz, rows);
    s.bar.wait();
    if (r == 0) {
        const auto o1 = Clock::now();
        file.AppendLayer(s.resVel.data(), s.resT.data());
        if (ms) { ms[0] += ms_between(o0, o1); ms[1] += ms_between(o1, Clock::now()); }
    }
    s.bar.wait();                                      // nobody writes the next record's rows while rank 0 still reads this one
}

// the reference's Profiler table (Common/Profiler.h:90-131: sorted by total time, events that never ran are absent; event
// names of AdiSolver3D.cpp:297-367, 555-680).  Device times from HIP events; MergeLayer has no launches of its own while
// the merge is fused into the sweep kernels; CreateSegments is the host time of the geometry upload.  Then the sweep kernels that ran.
template <typename FTYPE>
static void print_profiler_table(fs3d::AdiSolver3D<FTYPE> &solver, const RunOptions &o)
{
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
    int kx, ky, kz, sg;
    const char *kn[] = {"none", "line", "pipe", "part"};
    fs3d_last_sweep_kernel(solver.ctx(), 0, &kx, &sg); fs3d_last_sweep_kernel(solver.ctx(), 1, &ky, &sg); fs3d_last_sweep_kernel(solver.ctx(), 2, &kz, &sg);
    std::printf("Sweep kernels: X %s, Y %s, Z %s\n", kn[kx & 3], kn[ky & 3], kn[kz & 3]);
}

// the lines that close a run, up to the `steps in` line
template <typename FTYPE>
static void print_closing_lines(const Run<FTYPE> &s)
{
    const RunOptions &o = s.o;
    if (o.fresh_cells) {
        long long fresh = 0, filled = 0;
        for (int r = 0; r < s.nslabs; r++) { fresh += s.fresh_own[r]; filled += s.filled_own[r]; }
        std::printf("Fresh cells: %lld in %lld updates, %lld filled, at most %lld rounds\n", fresh, s.fresh_updates, filled, s.fresh_rounds);
    }
    if (o.time_geometry && s.steps > 0)                // (before the line of --time-both, which only a mesh has)
        std::printf(o.moving ? "Moving geometry per step (host clock, ms): Prepare %.3f, extrusion on the host %.3f, update call %.3f; step %.3f\n"
                             : "Moving mesh per step (host clock, ms): SubFrame %.3f, voxels on the host %.3f, update call %.3f; step %.3f\n",
                    s.geom_ms[0] / s.steps, s.geom_ms[1] / s.steps, s.geom_ms[2] / s.steps, s.sec * 1e3 / s.steps);
    if (o.time_both) {
        auto line = [](const char *what, std::vector<double> v) {
            if (v.size() <= 3) { std::printf(" %s: too few steps;", what); return; }
            v.erase(v.begin(), v.begin() + 3);
            std::sort(v.begin(), v.end());
            const size_t n = v.size();
            std::printf(" %s median %.3f min %.3f max %.3f n %zu;", what, n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]), v.front(), v.back(), n);
        };
        std::printf("Moving mesh, both paths per call (ms):");
        line("host voxels + fs3d_update_nodes", s.ab_host); line("fs3d_update_nodes_shape3d", s.ab_dev); line("its device time", s.ab_dev_gpu);
        line("time step", s.ab_step);
        std::printf(" fill rounds %d\n", s.fill_rounds);
    }
    if (o.time_output && s.nc.NumRecords() > 0)
        std::printf("Result output per record (host clock, ms): GetLayer %.3f, AppendLayer %.3f; %u records\n", s.out_ms[0] / s.nc.NumRecords(),
                    s.out_ms[1] / s.nc.NumRecords(), s.nc.NumRecords());
    std::printf("%ld steps in %.3f s: %.1f Mcells/s; %u layers in %s\n", s.steps, s.sec,
                (double)s.grid.dimx * s.grid.dimy * s.grid.dimz * s.steps / s.sec / 1e6, s.nc.NumRecords(), s.out.c_str());
}

// What rank r of the run does: its solver over its planes, the time loop, the statistics records.  On one rank every `r == 0` holds
// and every barrier is a barrier of one.  On several, rank 0 prepares the geometry of time t on the host, a barrier, then every rank
// updates its solver from it; after the step ClearOutterCells on every rank, and a barrier before rank 0 prepares the next geometry
// in the arrays the others have read.
template <typename FTYPE>
static void run_rank(Run<FTYPE> &s, const int r)
{
    using namespace fs3d;
    const RunOptions &o = s.o;
    const Config &cfg = s.cfg;
    const int nslabs = s.nslabs;
    const int q = s.grid.dimx / nslabs, rem = s.grid.dimx % nslabs;
    const int x0 = r * q + std::min(r, rem), x1 = x0 + q + (r < rem ? 1 : 0);
    AdiSolver3D<FTYPE> solver;
    solver.Init(nslabs == 1 ? o.device : o.same_device ? 0 : r, s.grid, s.params, x0, x1);
    if (nslabs > 1) solver.JoinLocalGroup(s.group, r);
    apply_options(solver, o, nslabs);
    // every rank has uploaded the grid of time 0 before rank 0 writes the next geometry into the same arrays (Init
    // reads them, and joining the group is no rendezvous)
    if (o.moves()) s.bar.wait();
    if (nslabs == 1) {
        std::printf("Segments: %i %i %i (x, y, z)\n", solver.numSegs[0], solver.numSegs[1], solver.numSegs[2]);
        s.create_result_file(s.nc, s.out);             // (after Init: a run that finds no GPU leaves no file)
        solver.EnableTiming(true);
        s.t0 = Clock::now();
    } else if (r == 0) std::printf("Slabs: %d x-slabs of %d..%d planes\n", nslabs, q, q + (rem ? 1 : 0));

    double t = s.dt;
    long steps = 0;
    int lastframe = -1;
    // without a moving word the geometry is frame 0's for the whole run: the reference prepares the grid once, before the loop
    // (grid->Prepare(0), :226; the per-step grid->Prepare(t) is commented out, :237) -- the frame only restarts the substep counter
    for (int i = 0; t < s.finaltime && (o.max_steps < 0 || steps < o.max_steps); t += s.dt, i++, steps++) {
        const int currentframe = s.geo.GetFrame(t);                                                      // :229-236
        if (currentframe != lastframe) { lastframe = currentframe; i = 0; }
        if (o.moves()) {
            if (o.time_both) {                         // a measurement run: the other path first, the word's own last (same tables either way)
                const auto b0 = Clock::now();
                prepare_geometry(s, t, !o.on_host());
                update_geometry(s, solver, !o.on_host());
                (o.host_voxels ? s.ab_dev : s.ab_host).push_back(ms_between(b0, Clock::now()));
            }
            const auto g0 = Clock::now();
            auto g1 = g0;
            if (r == 0) prepare_geometry(s, t, o.on_host(), &g1);
            s.bar.wait();
            const auto g3 = Clock::now();
            update_geometry(s, solver, o.on_host());
            const auto g4 = Clock::now();
            if (o.fresh_cells) {                       // the cells this update turned fluid, all ranks together, before UpdateBoundaries
                long long info[4];
                solver.FillFreshCells(info);
                s.fresh_own[r] += info[0]; s.filled_own[r] += info[1];
                if (r == 0) { s.fresh_updates++; s.fresh_rounds = std::max(s.fresh_rounds, info[2]); }
            }
            if (o.time_geometry) { s.geom_ms[0] += ms_between(g0, g1); s.geom_ms[1] += ms_between(g1, g3); s.geom_ms[2] += ms_between(g3, g4); }
            if (o.time_both) (o.host_voxels ? s.ab_host : s.ab_dev).push_back(ms_between(g0, g4));
        }
        if (o.time_both) {
            // (with --host-voxels the device path ran first: its device time was overwritten by the host path's update)
            float dms = 0;
            if (!o.host_voxels && fs3d_last_update_device_ms(solver.ctx(), &dms) == FS3D_OK) s.ab_dev_gpu.push_back(dms);
            fs3d_mesh_fill_rounds(solver.ctx(), &s.fill_rounds);
            fs3d_synchronize(solver.ctx());
        }
        const auto s0 = Clock::now();
        solver.UpdateBoundaries();                                                                       // :244
        solver.TimeStep((FTYPE)s.dt, cfg.num_global, cfg.num_local, (i % 10 == 0) || (t + s.dt >= s.finaltime)); // :245
        if (o.time_both) { fs3d_synchronize(solver.ctx()); s.ab_step.push_back(ms_between(s0, Clock::now())); }
        if (r == 0) {
            const float perres = (float)t * 100 / (float)s.finaltime;                                    // PrintTimeStepInfo, IO.h:455-478
            std::printf("\rerr = %.8f, frame %i\tsubstep %i\t%i%%", solver.diffError, currentframe, i, (int)perres);   // AdiSolver3D.cpp:376
            if (nslabs == 1 && perres < 2) std::printf("\t(----- left)");
            else if (nslabs == 1) {
                const float left = std::chrono::duration<float>(Clock::now() - s.t0).count() * (100 - perres) / perres;
                std::printf("\t(%i h %i m %i s left)", ((int)left) / 3600, (((int)left) / 60) % 60, ((int)left) % 60);
            }
            std::fflush(stdout);
        }
        if ((i % cfg.out_time_steps) == 0) record(s, solver, r, s.nc, s.out_ms);                          // :254-264
        if (o.moves()) { solver.ClearOutterCells(); s.bar.wait(); }      // AdiSolver3D.cpp:382-385; every rank has read this step's geometry
    }
    s.bar.wait();                                      // every rank is through its steps: the clock of the `steps in` line stops here
    if (r == 0) { s.steps = steps; s.sec = std::chrono::duration<double>(Clock::now() - s.t0).count(); }
    if (nslabs == 1) { print_profiler_table(solver, o); print_closing_lines(s); }    // (one GPU: before the statistics records)
    if (o.time_stats && steps > 0) {
        if (r == 0) s.create_result_file(s.ns, s.stats);
        for (const StatsRecord &rec : stats_records(o)) {
            solver.SetOutputSource(rec.source);
            if (o.time_cov) solver.SetOutputMoment(rec.moment);
            if (o.time_grad) solver.SetOutputGradient(rec.gradient);
            if (o.time_wall) solver.SetOutputWall(rec.wall);
            record(s, solver, r, s.ns, nullptr);
        }
        solver.SetOutputSource(0);
    }
}

template <typename FTYPE>
static int run_loop(fs3d::Grid3D<FTYPE> &grid, fs3d::Grid2D &g2, fs3d::Shape3D &sh3, const RunGeom &geo, const std::string &prefix,
                    const fs3d::Config &cfg, const RunOptions &o)
{
    Run<FTYPE> s(grid, g2, sh3, geo, prefix, cfg, o);
    const int nslabs = s.nslabs;
    if (nslabs == 1) run_rank(s, 0);                   // on the calling thread: no group, no thread
    else {
        s.create_result_file(s.nc, s.out);
        s.group = fs3d::AdiSolver3D<FTYPE>::CreateLocalGroup(nslabs);
        std::vector<std::exception_ptr> errs(nslabs);
        std::vector<std::thread> th;
        s.t0 = Clock::now();
        for (int r = 0; r < nslabs; r++)
            th.emplace_back([&, r] {
                try { run_rank(s, r); }
                catch (...) {
                    // release the other slab threads: they wait for this one in the transport (halo planes, carries) or at a
                    // barrier and would never return
                    errs[r] = std::current_exception();
                    fs3d_local_group_abort(s.group);
                    s.bar.abort();
                }
            });
        for (auto &t : th) t.join();
        fs3d::AdiSolver3D<FTYPE>::DestroyLocalGroup(s.group);
        for (auto &e : errs) if (e) {          // the first failure, not the "another slab thread failed" it caused
            try { std::rethrow_exception(e); } catch (std::exception &x) { if (std::string(x.what()).find("another slab thread") == std::string::npos && std::string(x.what()).find("a peer failed") == std::string::npos) throw; } catch (...) { throw; }
        }
        for (auto &e : errs) if (e) std::rethrow_exception(e);
        std::printf("\n");
        print_closing_lines(s);
    }
    if (o.time_stats) {
        // steps: the time steps of the run; the line names the accumulated ones, the 1st, (K + 1)th, .. of them
        if (s.steps > 0) std::printf("Time statistics: %ld steps, mean%s%s%s%s in %s\n", (s.steps + o.time_every - 1) / o.time_every,
                                     o.time_stats == 2 ? ", variance" : "", o.time_cov ? ", covariances" : "", o.time_grad ? ", gradients" : "",
                                     o.time_wall ? ", wall" : "", s.stats.c_str());
        else std::printf("Time statistics: 0 steps, no file\n");
    }
    return 0;
}

template <typename FTYPE>
static int run(const std::string &data, const std::string &prefix, const fs3d::Config &cfg, const RunOptions &o)
{
    check_words(o, cfg);
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
    return run_loop<FTYPE>(grid, g2, sh3, geo, prefix, cfg, o);
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::printf("Usage: %s %s\n", argv[0], USAGE);
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
            else if (s == "--output-filter" || s == "--slab-output-filter") {       // one check for the argument of both words
                const std::string w = a + 1 < argc ? argv[++a] : "";
                if (w != "point" && w != "box") throw std::runtime_error("--output-filter: point or box");
                o.output_box = w == "box";
                o.slab_output_box = o.output_box && s == "--slab-output-filter";
            }
            else if (s == "--time-stats") {
                const std::string w = a + 1 < argc ? argv[++a] : "";
                if (w != "mean" && w != "variance") throw std::runtime_error("--time-stats: mean or variance");
                o.time_stats = w == "mean" ? 1 : 2;
            }
            else if (s == "--time-covariances") o.time_cov = true;
            else if (s == "--time-gradients") o.time_grad = true;
            else if (s == "--time-wall") o.time_wall = true;
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
        // (std::invalid_argument, caught below as every std::exception: the cases of these two refusals are in
        // tests/test_gradient_invariants_twin.py; the call-by-call matrix of tests/driver_calls.py lists the std::runtime_error sites)
        if (o.time_grad && !o.time_stats) throw std::invalid_argument("--time-gradients: needs --time-stats mean or --time-stats variance");
        if (o.time_grad && o.nslabs > 1)
            throw std::invalid_argument("--time-gradients: single GPU only (the gradient sums read a cell's neighbours in `cur`, whose ghost planes are not "
                                     "current after a step, and the library refuses them on an x-slab)");
        // (std::invalid_argument as the two above; their cases are in tests/test_wall_loads_twin.py)
        if (o.time_wall && !o.time_stats) throw std::invalid_argument("--time-wall: needs --time-stats mean or --time-stats variance");
        if (o.time_wall && o.nslabs > 1)
            throw std::invalid_argument("--time-wall: single GPU only (the wall sums read a wall cell's fluid neighbours in `cur`, whose ghost planes are not "
                                        "current after a step, and the library refuses them on an x-slab)");
        if (o.output_box && !o.slab_output_box && o.nslabs > 1)
            throw std::runtime_error("--output-filter box: single GPU only (with GPU n the grid is cut into x-slabs, a sample's box of source cells can "
                                     "straddle a cut, and the library refuses filtered records on a slab)");
        return o.dbl ? run<double>(argv[1], argv[2], cfg, o) : run<float>(argv[1], argv[2], cfg, o);
    } catch (std::exception &e) {
        std::fprintf(stderr, "\n\nCaught exception:\n%s\n\nTerminating...\n", e.what());     // FluidSolver3D.cpp:313-318
        return -1;
    }
}
