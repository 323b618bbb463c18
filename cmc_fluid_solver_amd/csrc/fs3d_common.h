// Shared declarations of the HIP implementation behind include/fs3d.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fs3d.h"
#include "fs3d_buf.h"         // OwnedBuf: the one owner of a device or pinned allocation
#include "fs3d_tables.h"      // the cell-code word, its row-code constants, UCOL_PITCH; the host definition of the geometry tables

// the two kinds of memory a context owns (fs3d_buf.h); a failed allocation leaves the runtime's error for the caller's text
struct DevMem {
    static void *alloc(size_t bytes) { void *p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static void *alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <class T = void> using DevBuf = OwnedBuf<DevMem, T>;
template <class T = void> using PinnedBuf = OwnedBuf<PinnedMem, T>;

template <typename R>
struct SweepParams {
    // geometry
    int dimx, dimy, dimz;       // owned planes
    long long plane;            // dimy*dimz
    // layers: one allocation per layer, field v at + v*fstride; the pointers address the first
    // OWNED cell of field 0 (one halo plane precedes every field).  Few pointers = few SGPRs.
    const R *cur_;
    const R *temp_;             // temp read by the stencils (old temp)
    R *next_;
    R *temp_out_;               // merged temp (== temp_ when not double-buffered)
    long long fstride;          // elements between consecutive fields of a layer
    const uint16_t *code;
    const uint8_t *dead;        // per line of the sweep direction: 1 = no cell of the line is on a segment or NODE_IN (partition kernels)
    // (r3) shared code columns of the X / Y partition kernels: where every live line of a group of 32 neighbouring lines carries the
    // same row codes (a box: all of them), the group reads ONE column of codes instead of 2 bytes per cell from HBM
    const uint16_t *ucol;       // [column id][UCOL_PITCH] the distinct columns (bits as in `code`), or nullptr -- a box has three of them: hot in the caches
    const unsigned *uflag;      // [o][group]: bit 0 the group is uniform, bit 1 so is the pair (group, group + 1) with equal columns (64-line tiles),
                                // bits 2.. the id of the group's (pair's) column
    int ung;                    // groups per row / plane: ceil(dimz / 32)
    const R *node_;             // node boundary values (v.x, v.y, v.z, T), field v at + v*nstride
    R *scr_;                    // LINE kernel scratch: c'_uvw, c'_T, d'_U, d'_V, d'_W, d'_T at + v*nstride
    long long nstride;          // elements between consecutive fields of node_ / scr_ (>= number of owned cells)
    __host__ __device__ const R *cur(int v) const { return cur_ + v * fstride; }
    __host__ __device__ const R *temp(int v) const { return temp_ + v * fstride; }
    __host__ __device__ R *next(int v) const { return next_ + v * fstride; }
    __host__ __device__ R *temp_out(int v) const { return temp_out_ + v * fstride; }
    __host__ __device__ const R *node(int v) const { return node_ + v * nstride; }
    __host__ __device__ R *scr(int v) const { return scr_ + v * nstride; }
    // constants, all rounded exactly as the reference's FTYPE expressions
    R two_ds[3];                // 2*dx, 2*dy, 2*dz            (TimeLayer3D.h:338-340)
    R vis_v, vis_t;             // v_vis/(ds*ds), t_vis/(ds*ds) (AdiSolver3D.cpp:744-751) for the sweep axis
    R b_v, b_t;                 // 3/dt + 2*vis                 (AdiSolver3D.cpp:761)
    R dt;
    R v_T, t_phi;
    unsigned long long *stamps; // measurement only: per-wave phase time stamps (s_memtime), or nullptr
    // x-slab halves of the X sweep (kernels_line.hip k_xsweep_*, kernels_pipe.hip MODE 1/2); null/0 otherwise
    const R *carry_in; R *carry_out; const R *xcarry_in; R *xcarry_out;
    int ghost_lo, ghost_hi;     // a neighbouring slab's plane stands before / behind the owned planes (X sweep stencils may read it)
    int bundle0;                // first bundle of this launch (line block of the cross-slab pipeline)
    int seg_index, scr_bundles; // halves: scratch slot = seg_index * scr_bundles + bundle
    int seg_begin, seg_len;     // halves: segment of the line this launch works on (seg_len 0: the whole line)
    long long carry_pitch;      // lines per value row of the carry arrays
    int fast_div;               // pipe kernel, fp32: constant divisors are in the range of the division core (kernels_pipe.hip)
    int merge;                  // 0: write next only; 1: also temp_out = merged; 2: merged twice (sweep merge + global merge)
    int o_begin, o_count;       // partition kernels: only the planes [o_begin, o_begin + o_count) of the slab (Y and Z sweeps; o_count 0: all) --
                                // interior planes run beside the halo exchange, the two edge planes after it
    int *errw;                  // device-visible error word (pinned host memory): bit 0 = a relay hand-over of the pipe kernel timed out
    int xiface_pass;            // X partition kernel on an x-slab: 1 = first pass, the slab's 18 interface words per line -> carry_out (pitch carry_pitch)
    int test_drop;              // test hook (env FS3D_TEST_DROP_HANDOFF): one wave never signals its hand-over; the poll bound is short
    int store_next;             // pipe kernel, fused time step: 0 when a later local iteration overwrites `next` unread (only the merge uses x)
};

#define FS3D_XREDUCE_MAX_RANKS 64      // k_xreduce (kernels_line.hip) holds the R x R slab system of a line in per-thread arrays of this size

// moving geometry (kernels_geom.hip): what fs3d_update_nodes* keeps between calls, allocated by the first one
struct fs3d_geom {
    DevBuf<uint8_t> stage;                  // type, bc_vel, bc_temp of the host entry points, dimx_global * plane cells each: a slab context
                                            // (fs3d_update_nodes*_slab) keeps the byte arrays of the GLOBAL grid, its X lines are read from them
    DevBuf<int> lst[3];                     // per line of X / Y / Z: last index whose type is not NODE_IN (-1: none)
    DevBuf<uint16_t> col[2];                // [o][group][UCOL_PITCH]: every group's candidate shared column (X, Y)
    DevBuf<uint8_t> cflag[2];               // [o][group]: bit 0 uniform, bit 1 the pair is
    DevBuf<unsigned long long> hash[2];     // [o][group]: hash of the column, for the identity decision on the host
    DevBuf<int> rep[2];                     // [column id]: the group whose column it is
    DevBuf<unsigned long long> cnt;         // counter words of one update
    PinnedBuf<> host;                       // pinned: counters, hashes, flags on their way to / from the host
    // extrusion of a Shape2D grid (k_geom_extrude): the per-column records, allocated by the first call.  One pinned block and its
    // device copy, dimx*dimy columns each: velx, vely, T (float), cell (uint8) -- the 13 bytes per column that change with time --
    // then bottom (int), which changes with (dz, depth, depth_var) only
    PinnedBuf<> ex_host; DevBuf<> ex_dev;
    bool ex_bottom_valid = false;           // the bottom table on the device is the one of (ex_dz, ex_depth, ex_depth_var)
    double ex_dz = 0, ex_depth = 0, ex_depth_var = 0;
    // voxelisation of a Shape3D mesh (k_geom_raster_mesh, k_geom_fill_*): allocated by the first call, grown when a mesh has more
    // vertices or triangles.  One pinned block -- x, y, z and the velocities wx, wy, wz of mesh_vcap vertices (float), 3 * mesh_tcap indices (int), the counter
    // words on their way back -- and the device copies of its three parts; the indices travel again only when they differ from
    // the ones the pinned block holds
    PinnedBuf<> mesh_host;
    DevBuf<float> mesh_vert;
    DevBuf<int> mesh_idx;
    DevBuf<unsigned> mesh_cnt;
    DevBuf<unsigned> mesh_owner;            // the entries with wall velocities: per cell the smallest index of the triangles that set it (all ones: none)
    int mesh_vcap = 0, mesh_tcap = 0, mesh_ntri_dev = -1;   // mesh_ntri_dev: triangles of the index list on the device (-1: none)
    int mesh_fill_rounds = 0;               // rounds the last flood fill ran, the closing one without a change included
    // device time of one update (fs3d_last_update_device_ms): event pairs around every batch of launches between two synchronisations;
    // a full array is folded into ev_ms (its events have completed: every batch ends with a synchronisation)
    hipEvent_t ev[16] = {};
    int ev_n = 0;
    bool ev_open = false;
    float ev_ms = 0;
    float last_dev_ms = 0;
    // fresh cells (k_fresh_classify, k_fresh_round; fs3d_fill_fresh_cells*).  The snapshot belongs to FS3D_OPT_FRESH_CELLS: one byte per
    // cell, the node types of the geometry the last update replaced, allocated by the first update made with the option on.  The
    // fill's own buffers are allocated by the first fill, kept and only grown: the round tag of every cell, the compact list of the
    // fresh cells, the counter words (device, and pinned on their way back)
    DevBuf<uint8_t> prev_type;
    bool prev_valid = false;                // prev_type holds the types of the geometry before the one the tables describe now
    float snap_ms = 0;                      // device time of the copy that made it (counted with the fill that reads it)
    DevBuf<uint8_t> fill_tag;
    long long fill_tag_off = 0;             // bytes from fill_tag to the first owned cell's tag: 0, or on a slab of a group (FS3D_OPT_FRESH_CELLS_SLABS)
                                            // the ghost plane in front of the owned planes, rounded up to 8
    DevBuf<int> fill_list;
    long long fill_cap = 0;                 // entries fill_list holds
    DevBuf<unsigned> fill_cnt; PinnedBuf<unsigned> fill_host;
    DevBuf<double> fill_red; PinnedBuf<double> fill_red_host;   // the collective fill: two counts on their way through fs3d_comm_allreduce_sum2 (device, pinned)
    float last_fill_ms = 0;
};

struct fs3d_ctx {
    int device = 0;
    fs3d_precision prec = FS3D_F32;
    int dimx = 0, dimy = 0, dimz = 0, x_offset = 0, dimx_global = 0;
    double gdx = 0, gdy = 0, gdz = 0;
    double v_T = 1, v_vis = 0, t_vis = 0, t_phi = 0;
    bool have_params = false, have_nodes = false;
    size_t esize = 4;
    long long plane = 0, ncell = 0;
    long long nstride = 0;      // elements between the fields of the node-value / scratch arrays: ncell + padding
    // 5 layer buffers (cur,temp,half,next + spare temp for double-buffering)
    void *lay[5] = {};          // one allocation per layer buffer: 4 fields of fstride elements (lay_raw + a per-layer skew)
    DevBuf<> lay_raw[5];        // the allocations
    long long fstride = 0;      // ncell + 2*plane + padding (the fields / layers of one cell must not share their low address bits)
    int slot[4] = {0, 1, 2, 3}; // layer id -> buffer
    int spare = 4;
    DevBuf<uint16_t> code;
    DevBuf<uint16_t> ucol[2];   // shared code columns of the X / Y partition kernels (SweepParams::ucol)
    DevBuf<unsigned> uflag[2];
    DevBuf<uint8_t> dead[3];    // per direction, one byte per line: the line has no segment cell and no NODE_IN cell (X: [j][k], Y: [i][k], Z: [i][j])
    DevBuf<> node;              // 4 x ncell
    DevBuf<> scr;               // >= 6 x ncell: rows of the thread-per-line kernel / of the pipe kernel's halves (allocated on demand)
    // compact list of NODE_BOUND / NODE_VALVE cells (AdiSolver3D.cpp:286-311)
    DevBuf<int> bnd_idx;
    DevBuf<> bnd_val[4];
    int n_bnd = 0;
    int bnd_cap = 0;            // entries the list buffers hold (fs3d_update_nodes grows them, never shrinks)
    long long ucol_cap[2] = {0, 0};   // columns ucol[d] holds when fs3d_update_nodes allocated it (0: the upload's exact-size table)
    int n_ucol[2] = {0, 0};     // distinct shared columns
    bool uploaded_once = false; // fs3d_upload_nodes has succeeded: the fixed-size tables exist
    long long geom_allocs = 0;  // device allocations + frees made by fs3d_upload_nodes / fs3d_update_nodes* (fs3d_geometry_info)
    int n_create_segments = 0;  // successful uploads + updates
    fs3d_geom geom;
    int nseg[3] = {0, 0, 0};
    long long stale_in_cells = 0;  // NODE_IN cells on no segment of some direction (they merge stale `next` values): 0 for closed geometries
    // div error partials
    DevBuf<double> red_buf;
    PinnedBuf<double> red_host;
    int red_blocks = 0;
    double diffError = 0.0;
    // result output (fs3d_get_layer*): device staging of the samples on their way to the host -- the V part, then the T part at
    // a 256-byte boundary; grown when a call needs more, never shrunk
    DevBuf<> gl_stage;
    long long gl_info[FS3D_N_GETLAYER_INFO] = {0, 0, 0};   // fs3d_get_layer_info
    int test_drop = 0;             // fault-injection hook of tests/test_gpu_failures.py: env FS3D_TEST_DROP_HANDOFF, read ONCE at fs3d_create
    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;     // multi-GPU: halo planes travel here, beside the interior planes' sweep on `stream`
    hipStream_t xstream = nullptr;         // the stream the transport works on right now (stream or comm_stream)
    hipEvent_t ev_src = nullptr, ev_halo = nullptr;
    int opt_overlap = 1;                   // FS3D_OPT_OVERLAP
    int opt_keep_temp = 0;                 // FS3D_OPT_KEEP_TEMP
    int opt_f64_part = 0;                  // FS3D_OPT_F64_PART
    int opt_mesh_voxels = 0;               // FS3D_OPT_MESH_VOXELS: 0 = the reference's rasteriser, 1 = conservative voxelisation (k_geom_voxel_mesh)
    int opt_mesh_shell = 0;                // FS3D_OPT_MESH_SHELL: 0 = the conservative shell as it is, 1 = its thin (6-separating) subset (k_geom_voxel_mesh<.., true>)
    int opt_fresh_cells = 0;               // FS3D_OPT_FRESH_CELLS: 1 = every single-context update keeps the node types of the geometry it replaces
    int opt_fresh_slabs = 0;               // FS3D_OPT_FRESH_CELLS_SLABS: 1 = a slab of a group keeps that snapshot too and fills collectively
    int opt_out_filter = 0;                // FS3D_OPT_OUTPUT_FILTER: 1 = the GetLayer entries average the NODE_IN cells of every sample's box (k_get_layer_box)
    int opt_out_vector = 0;                // FS3D_OPT_OUTPUT_VECTOR: 1 = their outV holds the vorticity (k_get_layer_box with VEC 1)
    // FS3D_OPT_OUTPUT_SLABS: 1 = on a member of a group fs3d_get_layer_rows / _dev take the two options above as one collective call
    // (get_layer_impl with `collective`, kernels_output.hip).  Its buffers are allocated by the first call that needs them, kept and only grown, counted in gl_info[2]:
    // os_type -- four planes of node types, a byte per cell: the own first and last plane (derived from `code` per call), the lower
    // and the upper neighbour's; os_part -- the five partial sums per sample of the straddling rows, [row][4 sums, count][ody*odz];
    // os_cuts -- (x_offset, dimx) of every rank, gathered once through os_cut_dev (the cuts of a group never move)
    int opt_out_slabs = 0;
    DevBuf<uint8_t> os_type;
    DevBuf<double> os_part;
    DevBuf<> os_cut_dev;
    std::vector<int> os_cuts;
    // time statistics (kernels_stats.hip): per own cell, no ghost planes -- the steps it was NODE_IN (ts_n), the double sums of U, V, W, T
    // over those steps (ts_s1, field v at + v * ts_stride), in mode 2 of their squares (ts_s2) and, in mode 2 with
    // FS3D_OPT_TIME_STATS_CROSS, of the six products uv, uw, vw, uT, vT, wT (ts_sx, pair p at + p * ts_stride).  Each is allocated by
    // the first accumulation that needs it, counted in geom_allocs and kept over later windows; all are freed when FS3D_OPT_TIME_STATS is
    // set to 0, ts_sx also when the CROSS option is.  Every set of FS3D_OPT_TIME_STATS, _CROSS or _EVERY opens a new window: ts_steps and
    // ts_candidates 0, ts_clear.  A candidate is a step that reached fs3d_time_stats_accumulate (a successful fs3d_time_step, every
    // fs3d_time_step_async); candidate s = 1, 2, .. is accumulated where (s - 1) % opt_ts_every == 0, nothing runs on the others.
    // ts_q is the statistic layer of the read-out (4 fields of ts_stride reals), allocated by the first fs3d_get_layer* call with a
    // source other than 0 and kept; with source 2, opt_out_moment chooses the variances, the Reynolds stresses or the heat fluxes
    int opt_time_stats = 0;                // FS3D_OPT_TIME_STATS: 0 off, 1 first moments, 2 first and second moments
    int opt_ts_cross = 0;                  // FS3D_OPT_TIME_STATS_CROSS: 1 = mode 2 also accumulates the six cross sums
    int opt_ts_every = 1;                  // FS3D_OPT_TIME_STATS_EVERY: the stride k of the accumulated steps, 1 .. 2^20
    int opt_out_source = 0;                // FS3D_OPT_OUTPUT_SOURCE: 0 `next`, 1 time mean, 2 time variance, 3 fluid fraction
    int opt_out_moment = 0;                // FS3D_OPT_OUTPUT_MOMENT: what source 2 builds -- 0 variances, 1 Reynolds stresses and k, 2 heat fluxes and var_T
    long long ts_steps = 0;                // N: accumulated steps of the open window
    long long ts_candidates = 0;           // candidate steps of the open window, accumulated or not
    bool ts_clear = false;                 // the window is new: the next accumulation zeroes the accumulators first
    long long ts_stride = 0;               // ncell rounded up to 4 (every field of the accumulators starts on 16 bytes)
    DevBuf<unsigned> ts_n;
    DevBuf<double> ts_s1, ts_s2, ts_sx;
    DevBuf<> ts_q;
    // gradient sums (FS3D_OPT_TIME_STATS_GRAD; k_time_grad, kernels_stats.hip): per own cell the accumulated steps on which it carried
    // invariants (tg_n) and the double sums of div, Q and S:S over them (tg_g, quantity v at + v * ts_stride) -- 28 bytes per cell in
    // two buffers, allocated by the first accumulation that needs them, counted in geom_allocs, kept over windows, freed when this
    // option or FS3D_OPT_TIME_STATS is set to 0.  They share the window of the sums above (every set of the option opens a new one)
    // and are zeroed by the accumulation that zeroes those
    int opt_ts_grad = 0;                   // FS3D_OPT_TIME_STATS_GRAD: 1 = every accumulated step also sums the invariants of the velocity gradient
    int opt_out_gradient = 0;              // FS3D_OPT_OUTPUT_GRADIENT: outV of the GetLayer entries -- 1 the invariants of the sampled layer, 2 their time mean
    DevBuf<unsigned> tg_n;
    DevBuf<double> tg_g;
    // wall sums (FS3D_OPT_TIME_STATS_WALL; k_time_wall, kernels_stats.hip): per own cell the accumulated steps on which it was a
    // carrier of wall loads (tw_n) and the double sums of tau_x, tau_y, tau_z, |tau| and q over them (tw_w, quantity v at
    // + v * ts_stride) -- 44 bytes per cell in two buffers, with the life of the gradient sums above: allocated by the first
    // accumulation that needs them, counted in geom_allocs, kept over windows, freed when this option or FS3D_OPT_TIME_STATS is
    // set to 0, zeroed by the accumulation that opens a window
    int opt_ts_wall = 0;                   // FS3D_OPT_TIME_STATS_WALL: 1 = every accumulated step also sums the wall loads
    int opt_out_wall = 0;                  // FS3D_OPT_OUTPUT_WALL: outV of the GetLayer entries -- 1 tau, 2 (|tau|, q, area), 3 mean tau, 4 (tawss, mean q, osi)
    DevBuf<unsigned> tw_n;
    DevBuf<double> tw_w;
    int opt_err_order = 0;                 // FS3D_OPT_ERR_ORDER: 1 = EvalDivError sums its per-cell terms serially in cell order (host), as the CPU path
    DevBuf<double> err_terms;              // ... one term per cell (device, allocated on first use)
    std::vector<double> err_terms_host;
    DevBuf<double> err_parts;              // a member of a group: EvalDivError's per-workgroup (sum, count) pairs of ALL global planes (device, allocated on first use)
    // options
    int opt_kernel = FS3D_SWEEP_AUTO;
    int ran_kernel[3] = {0, 0, 0};   // per direction: the kernel the last sweep really ran (fs3d_last_sweep_kernel)
    int ran_segmented[3] = {0, 0, 0};
    int ran_launch[3][2][8] = {};    // per direction and pass: the partition kernel instance and launch of the last sweep (fs3d_last_sweep_launch)
    int opt_fuse = 1;
    // timing
    bool timing = false;           // events around the launches being enqueued now
    int timing_period = 0;         // fs3d_enable_timing(on): 0 off, 1 every time step, N every N-th time step (sampling)
    long timing_steps = 0;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    std::vector<int> ev_class;
    // device time per event of the reference's Profiler vocabulary (AdiSolver3D.cpp:297-367, 555-680): 0 SolveSegments_Z, 1 _Y, 2 _X,
    // 3 CopyLayer, 4 MergeLayer, 5 EvalDivError, 6 UpdateBoundaries, 7 syncHalos
    float t_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int t_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double t_create_segments_ms = 0;       // host time of fs3d_upload_nodes (CreateSegments + Init_GPU)
    DevBuf<unsigned long long> stamps;      // device buffer for fs3d_profile_sweep
    // comm
    void *comm = nullptr;          // ncclComm_t
    void *local = nullptr;         // fs3d_local_group* (in-process transport)
    DevBuf<> carry[4];             // cross-slab X sweep: fwd in/out (6 x plane), bwd in/out (4 x plane)
    int opt_div_core = 1;          // FS3D_OPT_DIV_CORE
    DevBuf<> seg_carry[2];         // segmented long-line sweeps: forward (2 x 6 x lines) and backward (4 x lines) carries
    DevBuf<int> redo;              // pipe kernel, fp32: per-bundle "compute again with full divisions" flags (all zero between sweeps)
    // pinned + mapped error word of the kernels (checked at every synchronisation).  The one allocation that is no OwnedBuf: mapped
    // memory with a device alias, made once by fs3d_create and freed by fs3d_destroy
    int *errw_host = nullptr, *errw_dev = nullptr;
    int rank = 0, nranks = 1;
    DevBuf<> xif_send, xif_all;    // reduced-interface X sweep: this slab's 18 words per line / all ranks'
    DevBuf<> xa2a[4];              // distributed interface solve: packed words out / in, boundary values out / in ([rank][words][lines per rank])
    int opt_xsolve = 0;            // FS3D_OPT_XSOLVE: 0 auto, 1 pipelined (bit-exact), 2 reduced interface
    int ran_xsolve = 0;            // what the last cross-slab X sweep ran: 1 pipelined, 2 reduced interface, 3 reduced interface with the interface words from the partition kernel
    int ran_xa2a = 0;              // ... and whether the interface solve was distributed over the ranks (two all-to-alls instead of one all-gather)
    int xblocks = 4;               // line blocks of the cross-slab X sweep pipeline (env FS3D_XBLOCKS)
    std::string err;
};

// ---- host helpers shared by fs3d_hip.hip, kernels_geom.hip, kernels_output.hip and fs3d_comm.hip ---------------------------------
// The error text of a call goes to its context; without one (fs3d_create, a NULL handle) to the thread's, for fs3d_last_error(NULL).
inline thread_local std::string g_create_err;
static inline fs3d_status fail(fs3d_ctx *c, fs3d_status st, const std::string &msg) { if (c) c->err = msg; else g_create_err = msg; return st; }
// gpuSafeCall (GPUplan.cpp:173-193): message carries the device id (-1 without a context) and the runtime's error text
static inline std::string call_failed(const fs3d_ctx *c, const char *call, const char *why)
{
    return "GPU " + std::to_string(c ? c->device : -1) + ": " + call + " failed: " + why;
}
#define HIPCHK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail((c), FS3D_ERR_HIP, call_failed((c), #call, hipGetErrorString(e_))); } while (0)
#define GTRY(call) do { const fs3d_status st_ = (call); if (st_) return st_; } while (0)
// f<float>(args) or f<double>(args), by the precision of context c
#define BY_PREC(c, f, ...) ((c)->prec == FS3D_F32 ? f<float>(__VA_ARGS__) : f<double>(__VA_ARGS__))

// blocks of 256 threads for n items, at most `cap` (the kernels stride over what is left)
static inline unsigned grid_for(long long n, int cap = 4096) { return (unsigned)std::max(1LL, std::min<long long>((n + 255) / 256, cap)); }

// a reserve / replace / reserve_all of the context's buffers that failed, as the status of the call.  The geometry paths
// (fs3d_upload_nodes, fs3d_update_nodes*, the fill) pass &c->geom_allocs to their device buffers: fs3d_geometry_info entry 13
#define BUFCHK(c, ok) do { if (!(ok)) return fail((c), FS3D_ERR_HIP, call_failed((c), #ok, hipGetErrorString(hipGetLastError()))); } while (0)
// reserve_all for the buffers the sweeps use: before one of them is freed to grow, what the stream still does with it finishes
static inline bool stream_reserve(fs3d_ctx *c, std::initializer_list<BufWant<DevMem>> set, bool *fresh = nullptr)
{
    for (const BufWant<DevMem> &w : set) if (w.buf->raw() && !w.buf->holds(w.bytes)) { hipStreamSynchronize(c->stream); break; }
    return reserve_all(set, nullptr, fresh);
}

// the first owned cell of field v of layer buffer buf
template <typename R> static inline R *fld(fs3d_ctx *c, int buf, int v) { return (R *)c->lay[buf] + (long long)v * c->fstride + c->plane; }
// A rank that fails anywhere in a collective sequence -- allocations included -- must not leave its neighbours blocked in their
// receives: it aborts the group (fs3d_comm_abort), the peers' pending and later exchanges return FS3D_ERR_COMM
struct AbortOnError { fs3d_ctx *c; fs3d_status *st; ~AbortOnError() { if (*st != FS3D_OK) fs3d_comm_abort(c); } };

// fs3d_hip.hip: what every entry that returns synchronised does after the wait -- the event pairs of the timed launches into
// t_ms / t_n, then the kernels' error word
void rec_collect(fs3d_ctx *c);
fs3d_status check_device_errors(fs3d_ctx *c);

// kernels_geom.hip
void fs3d_geom_destroy(fs3d_ctx *c);

// The invariants of the velocity gradient (FS3D_OPT_OUTPUT_GRADIENT, FS3D_OPT_TIME_STATS_GRAD; the rule: layer_output.py) from the
// nine central-difference quotients g[a][b] = d u_a / d x_b: (div, Q, S:S), every operation rounded once in R, in the rule's order.
// Shared by the record kernel (kernels_output.hip) and the accumulation (kernels_stats.hip), both built with -ffp-contract=off.
template <typename R>
static __device__ __forceinline__ void fs3d_invariants(const R (&g)[3][3], R &div, R &q, R &ss)
{
    const R h = R(0.5f);
    div = (g[0][0] + g[1][1]) + g[2][2];
    const R sxy = h * (g[0][1] + g[1][0]), sxz = h * (g[0][2] + g[2][0]), syz = h * (g[1][2] + g[2][1]);
    const R oxy = h * (g[0][1] - g[1][0]), oxz = h * (g[0][2] - g[2][0]), oyz = h * (g[1][2] - g[2][1]);
    ss = ((g[0][0] * g[0][0] + g[1][1] * g[1][1]) + g[2][2] * g[2][2]) + R(2) * ((sxy * sxy + sxz * sxz) + syz * syz);
    const R oo = R(2) * ((oxy * oxy + oxz * oxz) + oyz * oyz);
    q = h * (oo - ss);
}

// The wall loads (FS3D_OPT_OUTPUT_WALL, FS3D_OPT_TIME_STATS_WALL; the rule: layer_output.py wall_loads) of the cell l = (x, y, z) of a
// whole grid whose code word is cw: false where it is no carrier.  Else area, the sums divided by it -- tau, q -- from the exposed
// faces in the order x-, x+, y-, y+, z-, z+, every operation rounded once in R in the rule's order.  The face (d, -1) is exposed
// iff the cell below is NODE_IN and not the first of its line (the wall cell itself closes its run); the face (d, +1) iff the wall
// cell's row kind of direction d is ROW_START (the next cell is then an INTERIOR row).  Either way the cell's nibble of direction d
// is that of a START or END row and carries the FREE bits.  Every address is inside the grid.  Shared by the record kernel
// (kernels_output.hip) and the accumulation (kernels_stats.hip), both built with -ffp-contract=off and IEEE divide and sqrt.
template <typename R>
struct WallRule {
    R h[3], A[3], nu, kappa;               // R(dx), R(dy), R(dz); the face areas R(dy)*R(dz), R(dx)*R(dz), R(dx)*R(dy); R(v_vis), R(t_vis)
};

template <typename R>
static WallRule<R> fs3d_wall_rule(double dx, double dy, double dz, double v_vis, double t_vis)
{
    const R hx = (R)dx, hy = (R)dy, hz = (R)dz;
    return WallRule<R>{{hx, hy, hz}, {hy * hz, hx * hz, hx * hy}, (R)v_vis, (R)t_vis};
}

template <typename R>
static __device__ __forceinline__ bool fs3d_wall_loads(const WallRule<R> &w, const uint16_t *__restrict__ code, const R *U, const R *V,
                                                       const R *W, const R *T, long long l, int x, int y, int z, long long plane,
                                                       int dimz, int cw, R (&tau)[3], R &q, R &area)
{
    const int ty = (cw >> CODE_TYPE_SHIFT) & 3;
    if (ty != FS3D_NODE_BOUND && ty != FS3D_NODE_VALVE) return false;
    const R *const F[4] = {U, V, W, T};
    const int idx[3] = {x, y, z};
    const long long stride[3] = {plane, (long long)dimz, 1};
    R sum[4] = {R(0), R(0), R(0), R(0)};
    area = R(0);
    bool carrier = false;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int nib = (cw >> (4 * d)) & 0xF;
        const bool vel = !(nib & ROW_VELFREE), temp = !(nib & ROW_TEMPFREE);
#pragma unroll
        for (int s = -1; s <= 1; s += 2) {
            const long long p = l + s * stride[d];
            const bool face = s < 0 ? idx[d] >= 2 && ((code[p] >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN : (nib & 3) == ROW_START;
            if (!face) continue;
            carrier = true;
            area = area + w.A[d];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (c == d || !(c == 3 ? temp : vel)) continue;
                const R g = (F[c][p] - F[c][l]) / w.h[d];
                const R t = (c == 3 ? w.kappa : w.nu) * g;
                sum[c] = sum[c] + w.A[d] * t;
            }
        }
    }
    if (!carrier) return false;
    tau[0] = sum[0] / area; tau[1] = sum[1] / area; tau[2] = sum[2] / area;
    q = sum[3] / area;
    return true;
}

// mag of the rule: sqrt((tau_x*tau_x + tau_y*tau_y) + tau_z*tau_z), correctly rounded
static __device__ __forceinline__ float fs3d_wall_mag(const float (&t)[3]) { return sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]); }
static __device__ __forceinline__ double fs3d_wall_mag(const double (&t)[3]) { return sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]); }

// kernels_stats.hip: FS3D_OPT_TIME_STATS / _CROSS / _EVERY / _GRAD / _WALL, FS3D_OPT_OUTPUT_SOURCE / _MOMENT
// one candidate step of the window: where the stride takes it, one accumulation of FS3D_LAYER_CUR, enqueued on the context's stream
// (the first one allocates and clears); else nothing
fs3d_status fs3d_time_stats_accumulate(fs3d_ctx *c);
// the statistic layer of `source` (1 mean, 2 second moments -- `moment` 0 variance, 1 stresses, 2 heat fluxes --, 3 fluid fraction)
// into ts_q, enqueued; q_out: its four fields.  `ghost`: ts_q in the layout of a layer buffer, a ghost plane on either side of every
// field (the collective records of FS3D_OPT_OUTPUT_SLABS exchange them); *qstride_out: elements from field to field
fs3d_status fs3d_time_stats_layer(fs3d_ctx *c, int source, int moment, void *q_out[4], bool *grown, bool ghost = false,
                                  long long *qstride_out = nullptr);
// FS3D_OPT_OUTPUT_GRADIENT 2: the fields U, V, W of the statistic layer a source-1 call has just built (q: their first own cells,
// qstride apart) become the time means of div, Q and S:S from the gradient sums, enqueued behind it; T stays the mean of T
fs3d_status fs3d_time_stats_grad_layer(fs3d_ctx *c, void *q, long long qstride);
// FS3D_OPT_OUTPUT_WALL 3 / 4: the same for the time means of the wall loads from the wall sums -- `which` 3: the mean traction,
// 4: (tawss, the mean heat flux, osi)
fs3d_status fs3d_time_stats_wall_layer(fs3d_ctx *c, int which, void *q, long long qstride);
// all accumulators / the cross sums alone / the gradient sums alone / the wall sums alone; the caller has synchronised the stream
void fs3d_time_stats_free(fs3d_ctx *c);
void fs3d_time_stats_free_cross(fs3d_ctx *c);
void fs3d_time_stats_free_grad(fs3d_ctx *c);
void fs3d_time_stats_free_wall(fs3d_ctx *c);

// kernels_*.hip
// What a sweep launcher did.  NA: it does not cover these dims / this precision / this slab form -- the caller may try the
// next kernel.  FAILED: a HIP call failed and c->err says which -- the caller returns FS3D_ERR_HIP, nothing falls back.
enum class Launch { RAN, NA, FAILED };
template <typename R> void launch_sweep_line(fs3d_ctx *c, int dir, const SweepParams<R> &p);
template <typename R> Launch launch_sweep_pipe(fs3d_ctx *c, int dir, const SweepParams<R> &p);
// kernels_part.hip: partition (reduced-interface) solve, results to a stated tolerance (double: only with c->opt_f64_part,
// and never for a slab)
template <typename R> Launch launch_sweep_part(fs3d_ctx *c, int dir, const SweepParams<R> &p);
// X sweep halves of an x-slab for the bundles [b0, b1) (64 lines each, line = j*dimz + k)
template <typename R> bool xslab_pipe_supported(const SweepParams<R> &p);
template <typename R> Launch launch_xslab_pipe(fs3d_ctx *c, SweepParams<R> p, int half, int b0, int b1);
// lines longer than the pipe kernel holds: the sweep as a sequence of segment halves on one GPU
template <typename R> Launch launch_sweep_pipe_segmented(fs3d_ctx *c, int dir, SweepParams<R> p);
template <typename R> void launch_xsweep_fwd(fs3d_ctx *c, const SweepParams<R> &p, const void *carry_in, void *carry_out, long long l0, long long l1);
// reduced-interface cross-slab X sweep: interface coefficients of this slab (18 words per line), the R x R interface solve
template <typename R> void launch_xiface(fs3d_ctx *c, const SweepParams<R> &p, void *out);
template <typename R> void launch_xreduce(fs3d_ctx *c, const void *all, long long nl, int nranks, int me, void *carry_in, void *xcarry_in);
template <typename R> void launch_xpack(fs3d_ctx *c, const void *in, long long nl, long long lp, void *out);
template <typename R> void launch_xreduce_a2a(fs3d_ctx *c, const void *all, long long nl, long long lp, int nranks, int me, void *out);
template <typename R> void launch_xunpack(fs3d_ctx *c, const void *in, long long nl, long long lp, void *carry_in, void *xcarry_in);
template <typename R> void launch_xsweep_bwd(fs3d_ctx *c, const SweepParams<R> &p, const void *xcarry_in, void *xcarry_out, long long l0, long long l1);
