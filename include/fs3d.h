/*
 * fs3d.h -- C ABI of the MI355X-native FluidSolver3D hot path (libfs3d_hip.so).
 *
 * This is the drop-in boundary.  The reference has no FFI layer; its backend seam
 * is the set of free functions the host classes call when hw == GPU and that the
 * .cu files define.  Each entry point below names the
 * reference interface it replaces (paths relative to /root/reference/src).
 *
 * Conventions
 *  - plain C types only; all arrays are host pointers unless the name says dev.
 *  - cell index = i*dimy*dimz + j*dimz + k, k unit-stride (TimeLayer3D.h:256-259).
 *  - "real" arrays are float when the context precision is FS3D_F32 and double
 *    when FS3D_F64 (the reference's compile-time FTYPE, Geometry.h:21).
 *  - every call returns an fs3d_status; fs3d_last_error() gives the message
 *    (the reference throws std::runtime_error from gpuSafeCall, GPUplan.cpp:173-193;
 *    the C++ host wrapper in cmc_fluid_solver_amd/host re-throws from the status).
 *  - calls are synchronous with respect to their results (as every reference
 *    launcher ends in deviceSynchronize, e.g. AdiSolver3D.cu:520) unless stated.
 *  - one context drives one GPU (one x-slab).  Multi-GPU = one process per GPU,
 *    one context each, joined by fs3d_comm_init (RCCL).
 */
#ifndef FS3D_H
#define FS3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fs3d_ctx fs3d_ctx;

typedef enum { FS3D_F32 = 0, FS3D_F64 = 1 } fs3d_precision;

typedef enum {
    FS3D_OK = 0,
    FS3D_ERR_INVALID = 1,      /* bad argument / call order */
    FS3D_ERR_HIP = 2,          /* HIP runtime error (message has device id + hip error) */
    FS3D_ERR_DIVERGED = 3,     /* diffError > ERR_THRESHOLD (AdiSolver3D.cpp:371-374 throws) */
    FS3D_ERR_UNSUPPORTED = 4,  /* geometry/feature outside what the kernels implement */
    FS3D_ERR_COMM = 5          /* RCCL error */
} fs3d_status;

/* Geometry.h:29-43 */
enum { FS3D_NODE_IN = 0, FS3D_NODE_OUT = 1, FS3D_NODE_BOUND = 2, FS3D_NODE_VALVE = 3 };
enum { FS3D_BC_NOSLIP = 0, FS3D_BC_FREE = 1 };
enum { FS3D_DIR_X = 0, FS3D_DIR_Y = 1, FS3D_DIR_Z = 2 };
/* the solver's four TimeLayer3D objects (AdiSolver3D.cpp:254-258) */
enum { FS3D_LAYER_CUR = 0, FS3D_LAYER_TEMP = 1, FS3D_LAYER_HALF = 2, FS3D_LAYER_NEXT = 3 };
enum { FS3D_VAR_U = 0, FS3D_VAR_V = 1, FS3D_VAR_W = 2, FS3D_VAR_T = 3 };

/* kernel selection for the line sweeps (fs3d_set_option(FS3D_OPT_SWEEP_KERNEL)) */
enum {
    FS3D_SWEEP_AUTO = 0,      /* fastest kernel that supports the dims: PART where it applies (fp32; fp64 only with
                                 FS3D_OPT_F64_PART, direction by direction), else as EXACT */
    FS3D_SWEEP_LINE = 1,      /* thread-per-line Thomas, c'/d' scratch in HBM (any dims); bit-equal to the CPU path */
    FS3D_SWEEP_PIPE = 2,      /* wave-pipelined Thomas, c'/d' in registers+LDS; bit-equal to the CPU path */
    FS3D_SWEEP_PART = 3,      /* partition (reduced-interface) solve: every chunk of a line eliminated at once; same
                                 equations, different rounding -- equal to the CPU path to a stated tolerance
                                 (DESIGN.md section 5), not bit for bit; errors where it does not apply (an fp64 context
                                 without FS3D_OPT_F64_PART; dims outside the kernels) */
    FS3D_SWEEP_EXACT = 4      /* fastest of the bit-exact kernels (PIPE, its segmented form, LINE) */
};  /* environment FS3D_DEFAULT_KERNEL=<id> sets the initial value of FS3D_OPT_SWEEP_KERNEL for new contexts */
enum {
    FS3D_OPT_SWEEP_KERNEL = 0,
    FS3D_OPT_FUSE_MERGE = 1,  /* 1 (default): merge fused into the sweep; 0: separate merge kernels */
    FS3D_OPT_OVERLAP = 4,     /* 1 (default): in a multi-GPU group the halo planes of a Y / Z sweep travel on a second stream beside the
                                 sweep of the interior planes, the two edge planes follow; 0: exchange first, then one launch */
    FS3D_OPT_XSOLVE = 3,      /* cross-slab X sweep of a multi-GPU group: 1 = pipelined over the ranks (the reference's form,
                                 AdiSolver3D.cu:524-640; bit-equal to one GPU), 2 = reduced interface (every rank eliminates its slab
                                 at once; equal to one GPU to rounding) with ONE all-gather per sweep, every rank solving every line's
                                 interface system, 3 = reduced interface with the interface solve distributed over the ranks (two
                                 all-to-alls of point-to-point transfers; bit-identical to 2), 0 (default) = 3 from three ranks on,
                                 2 for two ranks -- unless the sweep-kernel option asks for the bit-exact kernels (then 1) */
    FS3D_OPT_KEEP_TEMP = 5,   /* 0 (default): the merged temp of the LAST sweep of a fused time step is not computed or stored -- nothing
                                 reads it: the next step starts from temp := cur (AdiSolver3D.cpp:320), GetLayer and EvalDivError read
                                 `next`; FS3D_LAYER_TEMP then holds the iterate before that last merge.  1: store it, as the
                                 reference's private `temp` member holds it after TimeStep (the parity tests that download it) */
    FS3D_OPT_DIV_CORE = 2,    /* 1 (default): fp32 pipe kernel divides with the scaling-free core of the IEEE expansion and
                                 falls back to the full division where an operand needs scaling (same results); 0: always full */
    FS3D_OPT_F64_PART = 6,    /* fp64 contexts only (accepted and without effect in fp32).  0 (default): fp64 runs the bit-exact kernels,
                                 FS3D_SWEEP_PART fails with FS3D_ERR_UNSUPPORTED.  1: the fp64 partition kernels are open -- FS3D_SWEEP_AUTO
                                 runs them in every direction where they apply and falls back to the bit-exact kernels direction by
                                 direction where they do not; FS3D_SWEEP_PART runs them or fails, never falls back.  They apply to
                                 X / Y lines of 4..256 cells and to Z lines of 8..256 cells with dimz even and dimy >= 4 (longer
                                 lines: bit-exact kernels).  Results equal the CPU path to ~1e-15, not bit for bit.
                                 No effect on slab contexts (a multi-GPU group, or a context with a neighbouring slab's ghost planes):
                                 fp64 slabs keep the bit-exact Y / Z kernels and their cross-slab X solve.
                                 Environment FS3D_DEFAULT_F64_PART=1 sets the initial value for new contexts */
    FS3D_OPT_MESH_VOXELS = 8, /* how fs3d_update_nodes_shape3d and fs3d_voxelize_shape3d_dev turn a mesh into NODE_BOUND cells; no effect on
                                 any other entry.  0 (default): the reference's rasteriser, which is not watertight.  1: conservative
                                 voxelisation, closed for every closed mesh (the mesh section below).  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_FRESH_CELLS = 9, /* 0 (default): nothing changes anywhere.  1: every successful fs3d_update_nodes* call on a single context
                                 (on a slab of a group: together with FS3D_OPT_FRESH_CELLS_SLABS) first copies the node types of the
                                 geometry it replaces into a one-byte-per-cell buffer the context keeps (allocated by the first such update, counted in fs3d_geometry_info entry 13), which fs3d_fill_fresh_cells reads
                                 (the fresh-cell section below).  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_FRESH_CELLS_SLABS = 10, /* 0 (default): nothing changes anywhere -- an x-slab keeps no snapshot and fs3d_fill_fresh_cells* refuses
                                 it.  1, on an x-slab context that is a member of a group (fs3d_comm_init_local, or fs3d_comm_init with more
                                 than one rank): while FS3D_OPT_FRESH_CELLS is 1 the four fs3d_update_nodes*_slab entries keep the snapshot
                                 of the node types of the slab's own planes, under the single context's rules, and fs3d_fill_fresh_cells*
                                 run their collective form (the fresh-cell section below).  No effect on a single context; a lone slab
                                 of a larger grid, in no group, is still refused.  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_MESH_SHELL = 11, /* which cells of the conservative voxelisation (FS3D_OPT_MESH_VOXELS set to 1) become NODE_BOUND, for every mesh entry
                                 that voxelises (fs3d_update_nodes_shape3d, _vel, _slab, _vel_slab, fs3d_voxelize_shape3d_dev, _vel_dev).
                                 0 (default): nothing changes anywhere -- every cell whose closed unit box a triangle touches.  1: the thin
                                 shell -- of those, the cells whose centre cross (the three unit segments through the centre, one along each
                                 axis) a triangle meets: closed for the 6-neighbourhood of the fill, about 0.55 of the cells (the mesh section
                                 below).  A mesh entry called with 1 while FS3D_OPT_MESH_VOXELS is 0 fails with FS3D_ERR_INVALID before
                                 anything is touched.  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_FILTER = 12, /* how fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev turn `next` into samples; no effect on any
                                 other entry.  0 (default): nothing changes anywhere -- the reference's point sample (FilterToArrays).
                                 1: the box mean -- every sample is the mean over the NODE_IN cells of its box of source cells, and the
                                 point sample where the box holds none (the GetLayer section below).  While it is 1 an x-slab or a member
                                 of a group is refused by the three entries (FS3D_ERR_UNSUPPORTED) unless FS3D_OPT_OUTPUT_SLABS is 1.
                                 Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_VECTOR = 13, /* what outV of the same three entries holds; outT is the temperature either way.  0 (default): nothing
                                 changes anywhere -- the velocity.  1: the vorticity, central differences on the NODE_IN cells whose six
                                 neighbours are inside the grid and not NODE_OUT, 99999 on NODE_OUT cells, 0 elsewhere (the GetLayer
                                 section below); combines with either filter.  Slabs are refused as above.  Any other value:
                                 FS3D_ERR_INVALID */
    FS3D_OPT_TIME_STATS = 14, /* running time statistics of the fields (the time-statistics section below).  0 (default): nothing changes
                                 anywhere and nothing is allocated.  1: first moments -- while it is set, every fs3d_time_step that returns
                                 FS3D_OK and every fs3d_time_step_async adds the new FS3D_LAYER_CUR to per-cell sums, one kernel on the
                                 context's stream.  2: first and second moments.  EVERY call with this option opens a new window (no step
                                 accumulated yet, the sums count as zero); setting 0 also frees the accumulators.  Any other value:
                                 FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_SOURCE = 15, /* the layer fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev turn into samples.  0 (default):
                                 `next`, nothing changes anywhere.  1: the time mean, 2: the time variance, 3: the fluid fraction of the
                                 open window of FS3D_OPT_TIME_STATS (the time-statistics section below).  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_TIME_STATS_CROSS = 16, /* 0 (default): nothing changes anywhere and nothing is allocated.  1: while FS3D_OPT_TIME_STATS is 2,
                                 every accumulation also adds the six products uv, uw, vw, uT, vT, wT to six more per-cell double sums, in
                                 the same kernel (48 bytes per own cell); while the mode is 0 or 1 it has no effect and allocates nothing.
                                 EVERY call with this option opens a new window; setting 0 also frees the cross sums.  Any other value:
                                 FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_MOMENT = 17, /* which second-moment layer FS3D_OPT_OUTPUT_SOURCE 2 builds; read only when the source is 2.  0 (default):
                                 the four variances, nothing changes.  1: the Reynolds stresses cov(u,v), cov(u,w), cov(v,w) in outV and the
                                 turbulent kinetic energy in outT.  2: the turbulent heat fluxes cov(u,T), cov(v,T), cov(w,T) in outV and
                                 the variance of T in outT.  1 and 2 need the cross sums of the open window and exclude
                                 FS3D_OPT_OUTPUT_VECTOR 1 (the time-statistics section below).  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_TIME_STATS_EVERY = 18, /* the stride k of the accumulated steps, 1 (default) .. 2^20: of the candidate steps s = 1, 2, .. of a
                                 window those with (s - 1) % k == 0 are accumulated, on the others no kernel runs.  EVERY call with this
                                 option opens a new window.  Needs no memory.  A value below 1 or above 2^20: FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_SLABS = 19, /* 0 (default): nothing changes anywhere -- the slab refusal of FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR
                                 stands.  1: on an x-slab context that is a member of a group (fs3d_comm_init_local, or fs3d_comm_init with
                                 more than one rank) fs3d_get_layer_rows and fs3d_get_layer_dev take a non-zero filter or vector option and
                                 run as one COLLECTIVE call: the slab writes its rows of the record a single context of the GLOBAL grid
                                 writes (the GetLayer section below).  No effect on a whole-grid context and none while both options are 0.
                                 Still refused with FS3D_ERR_UNSUPPORTED before any launch and any word to a peer: a lone slab of a larger
                                 grid in no group, and fs3d_get_layer on any slab (it samples the slab's own planes and stays
                                 non-collective).  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_GRADIENT = 20, /* what outV of fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev holds, beside
                                 FS3D_OPT_OUTPUT_VECTOR; outT is the temperature either way.  0 (default): nothing changes anywhere, no
                                 launch differs.  1: the invariants of the velocity gradient of the sampled layer (`next`, or the statistic
                                 layer FS3D_OPT_OUTPUT_SOURCE names) in place of the velocity -- (div u, Q, S:S), central differences on the
                                 cells that carry a vorticity, 99999 on NODE_OUT cells, 0 elsewhere (the GetLayer section below).  Accepted
                                 and refused exactly where FS3D_OPT_OUTPUT_VECTOR 1 is, with the same statuses: it combines with either
                                 filter, is refused on an x-slab or group member unless FS3D_OPT_OUTPUT_SLABS is 1 (then the same
                                 collective call as the curl), by fs3d_get_layer on any slab, on a lone slab in no group, and with
                                 FS3D_OPT_OUTPUT_MOMENT 1 or 2 under source 2.  2: the time mean of the invariants from the gradient sums
                                 of FS3D_OPT_TIME_STATS_GRAD (the time-statistics section below); needs FS3D_OPT_OUTPUT_SOURCE 1 and an open
                                 window with those sums and an accumulated step, else the three entries return FS3D_ERR_INVALID before any
                                 launch.  1 or 2 while FS3D_OPT_OUTPUT_VECTOR is 1: the three entries return FS3D_ERR_INVALID (two options
                                 claim outV); fs3d_set_option accepts the two in either order.  Any other value: FS3D_ERR_INVALID, the
                                 option stays as it was */
    FS3D_OPT_TIME_STATS_GRAD = 21, /* 0 (default): nothing changes anywhere and nothing is allocated.  1: while FS3D_OPT_TIME_STATS is 1 or
                                 2, every accumulated step also enqueues one kernel, behind the step and the accumulation of the fields,
                                 that evaluates the invariants (div u, Q, S:S) of the velocity gradient of the new FS3D_LAYER_CUR on the
                                 cells that carry them and adds them to three per-cell double sums, with a per-cell count (28 bytes per
                                 own cell in two buffers; the time-statistics section below).  EVERY call with this option opens a new
                                 window; setting 0 also frees the gradient sums.  Whole-grid contexts only: on an x-slab (x_offset != 0 or
                                 dimx != dimx_global) the value 1 returns FS3D_ERR_UNSUPPORTED, and on a member of a group of more than one
                                 rank fs3d_time_step / fs3d_time_step_async return FS3D_ERR_UNSUPPORTED before any launch, without a swap
                                 and without counting a candidate, while this option and the mode are on.  Any other value:
                                 FS3D_ERR_INVALID */
    FS3D_OPT_OUTPUT_WALL = 22, /* what the flow does to the wall, in outV of fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev;
                                 outT is the temperature as ever.  0 (default): nothing changes anywhere, no launch differs.  1: the
                                 wall shear stress vector tau of the sampled layer (`next`, or the mean layer with
                                 FS3D_OPT_OUTPUT_SOURCE 1) on the wall cells that carry one; 2: (|tau|, the wall heat flux q, the exposed
                                 area) on the same cells; 99999 on NODE_OUT cells and 0 on every other cell (the GetLayer section below).
                                 With FS3D_OPT_OUTPUT_FILTER 1 the mean runs over the carriers of a box, not over its NODE_IN cells.
                                 3: the time mean of tau, 4: (the time-averaged |tau|, the time mean of q, the oscillatory shear index)
                                 from the wall sums of FS3D_OPT_TIME_STATS_WALL (the time-statistics section below); both need
                                 FS3D_OPT_OUTPUT_SOURCE 1 and an open window with those sums and an accumulated step, else the three
                                 entries return FS3D_ERR_INVALID before any launch.  Non-zero while FS3D_OPT_OUTPUT_VECTOR is 1 or
                                 FS3D_OPT_OUTPUT_GRADIENT is non-zero: the three entries return FS3D_ERR_INVALID (two options claim
                                 outV); fs3d_set_option accepts them in any order.  1 or 2 with FS3D_OPT_OUTPUT_SOURCE 2 or 3:
                                 FS3D_ERR_INVALID.  Non-zero on an x-slab or a member of a group: FS3D_ERR_UNSUPPORTED from the three
                                 entries, also with FS3D_OPT_OUTPUT_SLABS at 1.  Every refusal comes before any launch and leaves
                                 destinations, rows and layers untouched.  Any other value: FS3D_ERR_INVALID, the option stays as it was */
    FS3D_OPT_TIME_STATS_WALL = 23, /* 0 (default): nothing changes anywhere and nothing is allocated.  1: while FS3D_OPT_TIME_STATS is 1 or
                                 2, every accumulated step also enqueues one kernel, behind the step and the accumulation of the fields,
                                 that evaluates the wall loads of the new FS3D_LAYER_CUR on the wall cells that carry them and adds tau,
                                 |tau| and q to five per-cell double sums, with a per-cell count (44 bytes per own cell in two buffers;
                                 the time-statistics section below).  EVERY call with this option opens a new window; setting 0 also frees
                                 the wall sums.  Whole-grid contexts only, with the statuses of FS3D_OPT_TIME_STATS_GRAD: on an x-slab the
                                 value 1 returns FS3D_ERR_UNSUPPORTED, and on a member of a group of more than one rank fs3d_time_step /
                                 fs3d_time_step_async return FS3D_ERR_UNSUPPORTED before any launch, without a swap and without counting a
                                 candidate, while this option and the mode are on.  Any other value: FS3D_ERR_INVALID */
    FS3D_OPT_ERR_ORDER = 7  /* summation order of EvalDivError (fs3d_eval_div_error, fs3d_time_step with compute_error).  0 (default): the
                                 per-cell terms are summed in parallel (per workgroup, then over the workgroups; deterministic, equal to the
                                 CPU path to ~1e-12 relative).  1: they are summed one after the other in cell order, as the loop of
                                 TimeLayer3D::EvalDivError (TimeLayer3D.h:604-628) does -- on the bit-exact kernels the reported error then
                                 equals the CPU path's bit for bit, as the fields do.  Costs 8 bytes per cell of device memory, a copy of
                                 them to the host and a serial pass per evaluation; single context only (an x-slab: FS3D_ERR_UNSUPPORTED
                                 from the evaluation) */
};

/* ---- lifetime ---------------------------------------------------------------
 * Replaces GPUplan::init / multiDevAlloc of layers, scratch and tables
 * (GPUplan.cpp:35-77, AdiSolver3D.cpp:166-268 AdiSolver3D::Init).
 * dimx is the number of x-planes this context owns; x_offset/dimx_global place the
 * slab in the global grid (PARAplan::getOffset1D/getLength1D, PARAplan.cpp:71-126).
 * Single GPU: x_offset = 0, dimx_global = dimx.  dx,dy,dz are Grid3D::dx.. (double,
 * cast to FTYPE as TimeLayer3D does, TimeLayer3D.h:1078-1080). */
fs3d_status fs3d_create(fs3d_ctx **out, int device, fs3d_precision prec,
                        int dimx, int dimy, int dimz, double dx, double dy, double dz,
                        int x_offset, int dimx_global);
void fs3d_destroy(fs3d_ctx *ctx);
/* message of the last failing call on ctx (ctx == NULL: last fs3d_create failure) */
const char *fs3d_last_error(const fs3d_ctx *ctx);

/* FluidParams (Geometry.h:538-562) as passed by value into every sweep launch
 * (AdiSolver3D.h:40-41).  Values are the FTYPE members widened to double. */
fs3d_status fs3d_set_params(fs3d_ctx *ctx, double v_T, double v_vis, double t_vis, double t_phi);

fs3d_status fs3d_set_option(fs3d_ctx *ctx, int option, int value);

/* ---- geometry ---------------------------------------------------------------
 * Replaces Grid3D::Init_GPU (node-type upload, Grid3D.cpp:526-565) together with
 * AdiSolver3D::CreateSegments (AdiSolver3D.cpp:393-473, 553-562: segment lists and
 * NodesBoundary3D records built from the Node array and copied to the device).
 * Input is the slab's Node array as SoA (Grid3D.h:73-88): type, bc_vel, bc_temp
 * (uint8) and v.x, v.y, v.z, T (real).  Segment semantics are those of
 * Grid3D::GenerateListSegments (Grid3D.cpp:47-127); the device keeps them as per-cell
 * row codes instead of 40-byte Segment3D records.  n_seg_out[3] (optional) receives
 * the segment counts per direction X,Y,Z for cross-checking with the caller's lists.
 * All seven arrays cover the GLOBAL grid (dimx_global*dimy*dimz cells), as every rank of
 * the reference holds the whole Grid3D and clips global segments to its slab
 * (AdiSolver3D.cpp:475-524); the context keeps only its own planes. */
fs3d_status fs3d_upload_nodes(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel,
                              const uint8_t *bc_temp, const void *vx, const void *vy,
                              const void *vz, const void *T, int n_seg_out[3]);

/* ---- moving geometry ----------------------------------------------------------
 * AdiSolver3D::CreateSegments called again between time steps, after Grid3D::Prepare(t) has moved the walls (the reference's
 * 2D driver runs this loop, FluidSolver2D.cpp:130-133; the 3D classes carry it, AdiSolver3D.cpp:382-385).  Arguments and
 * meaning as fs3d_upload_nodes (global grid, SoA Node array, Grid3D::GenerateListSegments semantics), but every table the
 * sweeps read -- cell codes, dead-line bytes, shared code columns and their flags, node values, the BOUND / VALVE list, the
 * segment counts -- is rebuilt by kernels on the context's stream, and ends equal to what fs3d_upload_nodes would have built.
 * fs3d_update_nodes takes host arrays (seven copies into buffers the context keeps, then the device path),
 * fs3d_update_nodes_dev takes device arrays (same device as the context; read on the context's stream).
 *  - layers, options, params and timing are not touched.
 *  - only after a successful fs3d_upload_nodes (else FS3D_ERR_INVALID): the first geometry comes through the static path.
 *  - after the first call nothing is allocated or freed in steady state; the BOUND / VALVE list grows when a geometry
 *    exceeds its capacity and never shrinks.  Counts and flags (tens of bytes, and a few KB of column hashes) are read back.
 *  - one context = the whole grid: an x-slab (dimx != dimx_global, or a member of a group) gets FS3D_ERR_UNSUPPORTED
 *    ("single context only") from every entry whose name does not end in _slab.
 *  - a geometry that fs3d_upload_nodes refuses is refused with the same status.  The tables are rebuilt IN PLACE: after a
 *    refusal, or any failure half way, the context has NO geometry -- every call that needs nodes returns FS3D_ERR_INVALID
 *    ("upload nodes first") until an fs3d_upload_nodes or fs3d_update_nodes* succeeds.
 *  - host time of the call is added to the CreateSegments profiler event; its count is the number of uploads + updates.
 *
 * On x-slabs: the _slab entries -- fs3d_update_nodes_slab here, fs3d_update_nodes_shape2d_slab and
 * fs3d_update_nodes_shape3d[_vel]_slab in the two sections below -- rebuild the tables of a new geometry for the planes
 * [x_offset, x_offset + dimx) of the global grid.  No communication: as fs3d_upload_nodes does, every rank takes the GLOBAL input
 * and builds the tables of its own planes from it, with kernels on its own stream.  The call waits for no peer, so it is the same
 * for a lone slab context, a member of an in-process group and an RCCL rank; the caller makes it on every rank between the same
 * two time steps (and treats any rank's failure as fatal for the group, as for every other call).  A whole-grid context
 * (x_offset 0, dimx == dimx_global, no group) is accepted too and ends with the tables the entry without _slab builds.
 *  - fs3d_update_nodes_slab takes host arrays over the global grid, exactly as fs3d_upload_nodes takes them.  The three byte
 *    arrays travel whole; of the four value arrays only the slab's planes are read.
 *  - result: after FS3D_OK the context holds exactly what a fresh context of the same (x_offset, dimx, dimx_global) holds after
 *    fs3d_upload_nodes of the same arrays -- cell codes, dead lines (local: a slab whose piece of an X line holds only the line's
 *    END cell is live), shared columns, the BOUND / VALVE list, the node values, stale_in_cells; n_seg_out[0] counts the segments
 *    of the global X lines, [1] and [2] those of the slab's planes.  FS3D_ERR_UNSUPPORTED (a FREE cell that closes one segment and
 *    opens the next) exactly when that upload would return it: such a cell on ANY global X line, or on a Y / Z line of the
 *    slab's planes.
 *  - the rest is the list above, with two things stated more closely: a refusal that comes before the geometry is given up (NULL
 *    array, no upload yet, a bad Shape2D or mesh source) leaves the context unchanged and counts nothing, a geometry refused by
 *    the tables leaves no geometry; nothing is allocated or freed after a context's first slab update (the BOUND / VALVE list is
 *    grow-only).
 *  - cost: the staging buffer of a slab context holds the three byte arrays of the GLOBAL grid -- 3 bytes per global cell,
 *    allocated by the first slab update, never shrunk -- and every rank reads them for the X lines, so that pass does not shrink
 *    with the number of ranks; everything else works on the slab's planes.
 *  - not provided: a _dev form of the slab entries; shipping less than the global byte arrays. */
fs3d_status fs3d_update_nodes(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel,
                              const uint8_t *bc_temp, const void *vx, const void *vy,
                              const void *vz, const void *T, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_dev(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel,
                                  const uint8_t *bc_temp, const void *vx, const void *vy,
                                  const void *vz, const void *T, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_slab(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                   const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3]);
/* ---- moving geometry from a Shape2D grid: the extrusion on the device -------------
 * Grid3D::Prepare2D (Grid3D.cpp:608-668) after grid2D->Prepare(t): the 2D grid as it stands, extruded into the Node array by a
 * kernel.  What changes with time is the 2D grid -- per column (i, j) of the dimx x dimy plane, index i*dimy + j, the cell type
 * (uint8, one of FS3D_NODE_*) and velx, vely, T (float: Grid2D is float whatever the context's precision) -- 13 bytes per column
 * where fs3d_update_nodes ships 19 (fp32) or 35 (fp64) bytes per cell.  dz, depth, depth_var, baseT are Grid3D's constructor
 * arguments: active_dimz = ceil(depth / dz) + 1 cells of the context's dimz are inside the extrusion, the per-column `bottom`
 * (1 + (int)(depth_var * z * height), Grid3D.cpp:632-636) is computed on the host with the reference's expression, kept in the
 * context and uploaded again only when (dz, depth, depth_var) change.  The nodes equal those of the reference's loop cell for
 * cell, byte for byte, including the cells it writes several times (kernels_geom.hip states the rule as a priority list;
 * cmc_fluid_solver_amd/shape2d.py extrude_shape2d is its numpy twin).
 * All three entries return FS3D_ERR_INVALID before anything is launched, the context unchanged, for a NULL array, a cell2d value that
 * is not a node type, active_dimz below 2 or above dimz, and a depth_var that puts the `bottom` of a column that is not NODE_OUT
 * outside 0 .. dimz - 1 (where the reference's loop writes outside its array); the two without _slab FS3D_ERR_UNSUPPORTED for an
 * x-slab or group member.
 *
 * fs3d_extrude_shape2d_dev: the seven SoA node arrays (ncell elements each, on the context's device; real = the context's
 * precision) are written on the context's stream; returns synchronised.  The context's geometry is not touched (it needs none).
 * Fast path (4 cells per thread, 16-byte stores): dimz % 4 == 0, the three byte arrays aligned to 4 bytes and the four value
 * arrays to 16 bytes (fp32 and fp64 alike); any other dimz or alignment runs one cell per thread, same results.
 *
 * fs3d_update_nodes_shape2d: fs3d_update_nodes* with the extrusion as the source -- the 2D arrays go through a pinned buffer the
 * context keeps, the kernel writes type / bc_vel / bc_temp into the staging buffer of fs3d_update_nodes and the four value
 * fields into the node-value table, and the device path of fs3d_update_nodes_dev rebuilds every table.  Its contract is that of
 * fs3d_update_nodes* above in every line: after a first fs3d_upload_nodes only, single context only, a refused geometry gets
 * the upload's status and leaves NO geometry, nothing allocated after the first call, counted in CreateSegments, device time in
 * fs3d_last_update_device_ms.
 *
 * fs3d_update_nodes_shape2d_slab: the arguments and checks of fs3d_update_nodes_shape2d on an x-slab, under the contract of the
 * _slab entries above (result, refusals, cost); the 2D arrays cover dimx_global x dimy columns.  The extrusion runs on the device:
 * the byte arrays are written for all global columns, the value fields for the slab's planes. */
fs3d_status fs3d_extrude_shape2d_dev(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d,
                                     const float *T2d, double dz, double depth, double depth_var, double baseT,
                                     uint8_t *type_out, uint8_t *bc_vel_out, uint8_t *bc_temp_out, void *vx_out,
                                     void *vy_out, void *vz_out, void *T_out);
fs3d_status fs3d_update_nodes_shape2d(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d,
                                      const float *T2d, double dz, double depth, double depth_var, double baseT,
                                      int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape2d_slab(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d,
                                           const float *T2d, double dz, double depth, double depth_var, double baseT,
                                           int n_seg_out[3]);
/* The `bottom` table these entries use, dimx*dimy ints (index i*dimy + j); host only, no context, no GPU.  Test aid: the
 * table must equal the host loader's, whose (int) truncates a double product. */
fs3d_status fs3d_shape2d_bottom(int dimx, int dimy, double dz, double depth, double depth_var, int *bottom_out);
/* ---- moving geometry from a Shape3D mesh: voxelisation and flood fill on the device ------
 * Grid3D::Prepare3D_Shape (Grid3D.cpp:905-946) after ComputeSubframeInfo: Grid3D::Build (:859-903 -- RasterPolygon :709-789,
 * ProjectPointOnPolygon :688-707, RasterLine :791-811 for every triangle) and FloodFill (:813-857) by kernels, then the Node array
 * as Grid3D::Init / SetData leave it (:351-371, 818-838).  What changes with time is the sub-frame's vertex list: x, y, z (float,
 * nvert each) in GRID coordinates -- what host/Shape3D.h SubFrame(t) and shape3d.Shape3D.subframe(t) return -- and tri, 3 * ntri
 * indices into it; 12 bytes per vertex travel where fs3d_update_nodes ships 19 (fp32) or 35 (fp64) bytes per cell.  baseT is
 * Grid3D's constructor argument.  The rasteriser repeats every fp32 operation of host/Shape3D.h and its twin shape3d.py in their
 * order, so the nodes equal theirs cell for cell, byte for byte: type from the mesh, bc_vel = bc_temp = NOSLIP, v = 0, T = 0 on
 * NODE_BOUND cells and (real)(float)baseT elsewhere.  The result is a function of this call's mesh alone (stateless): the
 * reference's repeated Prepare_CPU leaves T = 0 on cells that once were walls, a value nothing reads after the layers have been
 * initialised -- the third stated deviation beside the two of host/Shape3D.h.
 * Every mesh entry returns FS3D_ERR_INVALID before anything is launched, the context unchanged, for a NULL array, nvert < 1,
 * ntri < 0, an index outside 0 .. nvert - 1 and a coordinate that is not finite or exceeds 65536 in magnitude (which keeps every
 * (int) defined and every line loop short); those without _slab FS3D_ERR_UNSUPPORTED for an x-slab or group member.
 * A mesh with a polygon scan line of more than 4 (dimx + dimy + dimz) + 16 cells (where shape3d.py raises and the reference
 * loops), or with a triangle so thin that its scan stops advancing in fp32, is refused with FS3D_ERR_INVALID after the rasteriser
 * has run: fs3d_update_nodes_shape3d then leaves NO geometry, the arrays of fs3d_voxelize_shape3d_dev hold no valid grid.
 *
 * Conservative voxelisation (FS3D_OPT_MESH_VOXELS set to 1).  The reference's rasteriser projects one point per scan cell back onto the
 * polygon and truncates: it can leave a gap in the NODE_BOUND shell of a closed mesh, the flood fill then runs through it and the
 * whole interior becomes NODE_OUT (an icosphere of 20 faces at radii 15 x 19 x 15 cells has no NODE_IN cell).  With the option on,
 * a cell is NODE_BOUND if and only if a triangle of the mesh overlaps the cell's CLOSED unit box [i, i+1] x [j, j+1] x [k, k+1] in
 * grid coordinates (a point p lies in cell floor(p), the reference's (int)p) -- a separating-axis triangle-box test on the fp32
 * vertices, evaluated in float64 (where the vertices local to the triangle's box and its edges are exact), whose every inequality
 * accepts with a slack far above its rounding bound (2^-34 of the triangle's size in cells: below 5e-7 of a cell whatever the
 * mesh, about 1e-9 for triangles a few cells wide; cmc_fluid_solver_amd/shape3d.py states rule and derivation), so rounding only
 * ever adds a cell.
 * Such a shell separates over the 26-neighbourhood: the 6-neighbour flood fill cannot cross the shell of a closed mesh.  It is up
 * to about three cells thick where the reference's is one or two, so the fluid volume is smaller than with the default.  The
 * nodes equal those of shape3d.Shape3D(voxels="conservative") and of host/Shape3D.h with voxels = 1 byte for byte (the host loader
 * and the kernels share one C++ text of the rule, csrc/fs3d_voxel.h; the numpy twin is its specification), and are a
 * function of this call's mesh alone.  This mode admits coordinates of at most 4096 grid cells in magnitude (FS3D_ERR_INVALID
 * before anything is launched, the context unchanged; the default mode keeps its 65536).  It has no scan lines: nothing is
 * refused after the kernels have run.  A triangle with two or three equal or collinear vertices sets the cells of its longest
 * edge; triangles and parts of triangles outside the grid are dropped.
 *
 * Thin shell (FS3D_OPT_MESH_SHELL set to 1, with FS3D_OPT_MESH_VOXELS set to 1).  The fill spreads over the 6-neighbourhood, so a
 * shell only has to keep apart two neighbouring cell centres whose connecting line a triangle cuts.  With the option on, a
 * triangle sets, of the cells its box test sets, those whose CENTRE CROSS it meets -- the three unit segments through the cell's
 * centre, one parallel to each axis (the same float64 values and slack, compared with the half-widths of the segment instead of
 * the box; cmc_fluid_solver_amd/shape3d.py states the rule and why it separates).  The shell of a closed mesh stays closed for
 * the fill, is a subset of the conservative one with about 0.55 of its cells, and every cell that was fluid stays fluid.
 * Degenerate triangles are treated as without the option.  In the _vel entries the owner of a wall cell is the triangle of
 * smallest index whose thin test sets it.  The nodes equal those of shape3d.Shape3D(voxels="conservative", shell="cross") and of
 * host/Shape3D.h with voxels = 1, shell = 1 byte for byte.  Every mesh entry that voxelises honours the option
 * (fs3d_update_nodes_shape3d, _vel, _slab, _vel_slab, fs3d_voxelize_shape3d_dev, _vel_dev); with it set while
 * FS3D_OPT_MESH_VOXELS is 0 they fail with FS3D_ERR_INVALID before anything is launched, the context unchanged.
 *
 * fs3d_voxelize_shape3d_dev: the seven SoA node arrays (ncell elements each, on the context's device; real = the context's
 * precision) are written on the context's stream; returns synchronised.  The context's geometry is not touched (it needs none).
 * Fast store path of the six arrays beside type as in fs3d_extrude_shape2d_dev (dimz % 4 == 0 and the arrays aligned).
 *
 * fs3d_update_nodes_shape3d: fs3d_update_nodes* with the voxelisation as the source -- the vertices go through a pinned buffer
 * the context keeps, the indices are uploaded again only when they differ from the last call's, the kernels write type / bc_vel /
 * bc_temp into the staging buffer of fs3d_update_nodes and the four value fields into the node-value table, and the device path
 * of fs3d_update_nodes_dev rebuilds every table.  Its contract is that of fs3d_update_nodes* above in every line: after a first
 * fs3d_upload_nodes only, single context only, a refused geometry gets the upload's status and leaves NO geometry, nothing
 * allocated after the first call (a mesh with more vertices or triangles than any before grows the buffers once), counted in
 * CreateSegments, device time in fs3d_last_update_device_ms.
 *
 * fs3d_flood_fill_dev: FloodFill alone on a device array of the context's dimx*dimy*dimz node types: cell (0,0,0) becomes
 * NODE_OUT whatever it was, NODE_OUT then spreads through NODE_IN cells over the 6-neighbourhood, every other value is a wall.
 * Returns synchronised; test and measurement aid.  fs3d_flood_fill_global_dev: the same for the GLOBAL grid, from any context (an
 * x-slab too) -- the fill the two _slab entries run: type_inout holds dimx_global * dimy * dimz node types on the context's
 * device, filled in place from global cell (0,0,0).  fs3d_mesh_fill_rounds: the rounds (three directional passes each) the last
 * fill on this context ran, the closing one that changed nothing included.
 *
 * Walls that carry the mesh's velocity and a temperature: fs3d_update_nodes_shape3d_vel / fs3d_voxelize_shape3d_vel_dev are
 * fs3d_update_nodes_shape3d / fs3d_voxelize_shape3d_dev with a velocity per vertex, wx, wy, wz (float, nvert each, in the solver's
 * velocity units: what host/Shape3D.h SubFrameVelocity(t) and shape3d.Shape3D.subframe_velocity(t) return), and wallT.  The
 * reference reads a velocity per vertex and interpolates it (Grid3D.cpp:915), then drops it in RasterPolygon / RasterLine: its
 * walls are at rest whatever the mesh does, and a wall that moves never pushes the fluid.  Here, with the conservative
 * voxelisation only (FS3D_OPT_MESH_VOXELS set to 1), whose overlap test defines it:
 *   owner     of a NODE_BOUND cell: the triangle of smallest index whose overlap test sets the cell (order-free: an integer
 *             minimum).  Where several triangles overlap a cell the choice is arbitrary; the velocity field of a mesh is continuous
 *             across shared vertices, so another choice moves the value by the velocity gradient times a cell.
 *   weights   float64 from the fp32 vertices, local to the cell's corner: the barycentric coordinates of the orthogonal projection
 *             of the cell's centre onto the owner's plane, clamped at 0 and normalised; a degenerate owner gives the clamped
 *             parameter of the projection onto its longest edge (cmc_fluid_solver_amd/shape3d.py states every operation).
 *   nodes     NODE_BOUND: bc_vel = bc_temp = NOSLIP, v = (w0 W0 + w1 W1) + w2 W2 per component rounded once to real,
 *             T = (real)(float)wallT; every other cell as without velocities (v = 0, T = (real)(float)baseT).
 * The nodes equal those of shape3d.nodes_of(.., wall_v, wall_T) and of host/Shape3D.h FillShape3DNodes byte for byte.  With all
 * velocities zero and wallT = 0 the seven arrays equal those of the entries without _vel byte for byte, and in every line the
 * contract is theirs.  More refusals, FS3D_ERR_INVALID before anything is launched, the context unchanged: FS3D_OPT_MESH_VOXELS
 * other than 1, a NULL velocity array, a velocity or wallT that is not finite.  The owner array (4 bytes per cell) is allocated
 * by the first call of a _vel entry, never in steady state.
 *
 * On x-slabs: fs3d_update_nodes_shape3d_slab / fs3d_update_nodes_shape3d_vel_slab take the arguments and checks of
 * fs3d_update_nodes_shape3d / fs3d_update_nodes_shape3d_vel, the vertices in GLOBAL grid coordinates, under the contract of the
 * _slab entries (the moving-geometry section above).  The fill is global -- NODE_OUT spreads from cell (0,0,0) of the GLOBAL
 * grid -- and the staging buffer of a slab update already holds the byte arrays of the global grid: every rank voxelises and
 * fills the global grid on its own device and asks nothing of a neighbour.  FS3D_OPT_MESH_VOXELS selects the rasteriser as above;
 * the _vel entry needs the conservative one.
 *  - result: what a fresh context of the same (x_offset, dimx, dimx_global) holds after fs3d_upload_nodes of the global nodes of
 *    the twin (shape3d.nodes_of / FillShape3DNodes of host/Shape3D.h; the _vel entry: with its wall velocities and wallT) --
 *    tables, node values and n_seg_out, byte for byte.
 *  - every refusal of the mesh itself (NULL array, no upload yet, an index outside the vertex list, a vertex that is not finite or
 *    lies past the coordinate bound, _vel without the conservative option, a velocity or wallT that is not finite) comes before
 *    the geometry is given up: the context is unchanged and nothing is counted.  A geometry refused after the kernels ran -- a
 *    scan line of the reference rasteriser past its bound; a shared FREE cell cannot occur, the walls are NOSLIP -- leaves no
 *    geometry until an update or upload succeeds.  A refusal's message starts with the entry's own name.
 *  - nothing is allocated or freed after a context's second call (the first brings the mesh buffers and, for _vel, the owner
 *    array -- 4 bytes per cell of the SLAB; a later call with a larger mesh grows the mesh buffers).
 *  - cost: rasterisation and flood fill run over the GLOBAL grid and are repeated on every rank, so that part of the device time
 *    does not shrink with the number of ranks -- the price of asking nothing of a neighbour.  The node kernel and the tables work
 *    on the slab's planes.  What travels is the mesh, 12 bytes per vertex (24 with velocities) and the index list when it
 *    changes, against 3 bytes per global cell and the value planes for a host voxelisation followed by fs3d_update_nodes_slab.
 *  - not provided: a _dev form; a fill shared between the ranks of a group; shipping less than the global byte arrays. */
fs3d_status fs3d_update_nodes_shape3d(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert,
                                      const int *tri, int ntri, double baseT, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape3d_vel(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                          const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                          double wallT, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape3d_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert,
                                           const int *tri, int ntri, double baseT, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape3d_vel_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                               const float *wy, const float *wz, int nvert, const int *tri, int ntri,
                                               double baseT, double wallT, int n_seg_out[3]);
fs3d_status fs3d_voxelize_shape3d_dev(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert,
                                      const int *tri, int ntri, double baseT, uint8_t *type_out, uint8_t *bc_vel_out,
                                      uint8_t *bc_temp_out, void *vx_out, void *vy_out, void *vz_out, void *T_out);
fs3d_status fs3d_voxelize_shape3d_vel_dev(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                          const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                          double wallT, uint8_t *type_out, uint8_t *bc_vel_out, uint8_t *bc_temp_out,
                                          void *vx_out, void *vy_out, void *vz_out, void *T_out);
fs3d_status fs3d_flood_fill_dev(fs3d_ctx *ctx, uint8_t *type_inout);
fs3d_status fs3d_flood_fill_global_dev(fs3d_ctx *ctx, uint8_t *type_inout);
fs3d_status fs3d_mesh_fill_rounds(fs3d_ctx *ctx, int *rounds_out);

/* ---- fresh cells: what a cell holds when a wall moves off it and it becomes NODE_IN ------
 * No reference counterpart (its per-step grid->Prepare(t) is commented out, FluidSolver3D.cpp:237).  Without these entries a cell
 * that turns NODE_IN starts from what its layer holds: (0, 0, 0, baseT) where it was NODE_OUT, the wall's node values where it was
 * NODE_BOUND / NODE_VALVE -- for a Shape3D mesh T = 0 against baseT in the fluid, in a shell of cells, every step.
 * The rule (cmc_fluid_solver_amd/fresh_cells.py fill_fresh_cells is its numpy twin, and the kernels equal it bit for bit): with
 * prev_type the node types before the update and the context's code table giving them now, a cell is a DONOR if it is NODE_IN in
 * both, FRESH if it is NODE_IN now and was not, and otherwise neither read nor written.  The fill runs in rounds r = 1, 2, ..: every
 * fresh cell still unfilled looks at its six neighbours in the order i-1, i+1, j-1, j+1, k-1, k+1 (outside the grid: skipped); a
 * neighbour counts if it is a donor or was filled in a round BEFORE r; with n >= 1 of them each of the four fields of `layer` becomes
 * (x1 + .. + xn) / (real)n -- summed in that order, every addition and the one division rounded in the context's precision, no fused
 * multiply-add, no reciprocal -- and the cell counts as filled in round r.  A round reads only the state before it, so nothing
 * depends on the order of the cells.  The fill ends after the first round that fills nothing or after max_rounds rounds
 * (0 = 250, the largest value; outside 0 .. 250: FS3D_ERR_INVALID).  Fresh cells that no chain of fresh cells joins to a donor keep
 * what they hold.  Every filled value lies between the smallest and the largest donor value of its field.
 * info[0] fresh cells, [1] filled, [2] rounds that filled at least one cell, [3] fresh cells left unfilled.
 *
 * fs3d_fill_fresh_cells_dev, the stateless form: prev_type_dev holds dimx*dimy*dimz node types on the context's device (aligned
 * to 8 bytes: 8 cells per thread in the classifying pass; else cell by cell, same results).
 * fs3d_fill_fresh_cells reads the snapshot of FS3D_OPT_FRESH_CELLS and returns FS3D_ERR_INVALID without a valid one: the option is
 * off (or was when the last update ran), no update has succeeded since the last fs3d_upload_nodes, or the update before the last
 * one failed and left no geometry to take the types from.
 * Both refuse before any launch and before any word to a peer, the context unchanged: a NULL argument, a bad layer, a bad
 * max_rounds, no nodes yet -- FS3D_ERR_INVALID; an x-slab or group member while FS3D_OPT_FRESH_CELLS_SLABS is 0 --
 * FS3D_ERR_UNSUPPORTED (single context only); with that option on, a lone x-slab of a larger grid that is in no group --
 * FS3D_ERR_UNSUPPORTED (it needs its neighbours).  Both work on the context's stream and return synchronised.  The round tag of
 * every cell (one byte), the compact list of the fresh cells and the counter words are allocated by the first fill, kept, and
 * only the list grows: counted in fs3d_geometry_info entry 13.  In a time loop the fill of FS3D_LAYER_CUR goes between the update
 * and fs3d_update_boundaries.
 * fs3d_last_fill_device_ms: device time of the last fill (as fs3d_last_update_device_ms: while fs3d_enable_timing is on, else 0);
 * for fs3d_fill_fresh_cells it includes the snapshot's copy kernel, which runs inside the update call but is not part of the
 * update's device time.
 *
 * On x-slabs (FS3D_OPT_FRESH_CELLS_SLABS set to 1 on every member of a group): the same two entries, as one COLLECTIVE call.  The
 * result is that of the rule above on the GLOBAL grid: after the call the planes of `layer` that each slab owns hold, bit for bit,
 * what the fill of a single context of the global grid leaves in those planes.  A neighbour on the plane before a slab's first
 * plane, or behind its last, counts exactly as an owned one; only the first slab's i-1 and the last slab's i+1 lie outside the grid.
 *  - contract: every rank of the group makes the call between the same two time steps, with the same `layer` and the same
 *    max_rounds (as it makes every fs3d_update_nodes*_slab call).  Every rank then makes the same exchanges and the same sums,
 *    whatever it holds: a slab without a single fresh cell takes part until the last round.
 *  - fs3d_fill_fresh_cells reads the slab's own snapshot, kept by the _slab update entries under the rules above;
 *    prev_type_dev of fs3d_fill_fresh_cells_dev holds the node types of the slab's dimx*dimy*dimz cells.
 *  - what travels: before every round, in one grouped exchange per rank, the boundary plane of the four fields of `layer` and one
 *    plane of round tags (a byte per cell) to and from either neighbour; once after the classifying pass and once per two rounds,
 *    two numbers summed over the ranks.  The ghost planes of `layer` are overwritten (every time step exchanges them again).
 *  - info[0], [1] and [3] count the rank's OWN cells, and their sums over the ranks are the numbers of the single context; info[2]
 *    is the number of rounds that filled a cell on ANY rank, the same on every rank and equal to the single context's.
 *  - a rank that fails inside the call (a HIP error, a transport error) aborts the group's transport as the other collective
 *    calls do (fs3d_comm_abort): its peers return FS3D_ERR_COMM from the exchange they wait in instead of waiting for ever.  The
 *    refusals listed above come before the first exchange; a caller that gives the ranks different arguments breaks the contract.
 *  - allocations: the first fill of a slab brings the tag array with a ghost plane on either side and two doubles for the sums,
 *    beside the single context's buffers; kept, counted in fs3d_geometry_info entry 13, nothing in steady state.  Set the option
 *    and join the group before the context's first fill.
 *  - fs3d_last_fill_device_ms is the device time of the rank's own kernels and copies; the transport's copies and the waits for
 *    the peers are not in it.
 *  - not provided: a lone slab; a fill that overlaps its exchange with the cells that have no neighbour across a cut. */
fs3d_status fs3d_fill_fresh_cells_dev(fs3d_ctx *ctx, const uint8_t *prev_type_dev, int layer, int max_rounds, long long info[4]);
fs3d_status fs3d_fill_fresh_cells(fs3d_ctx *ctx, int layer, int max_rounds, long long info[4]);
fs3d_status fs3d_last_fill_device_ms(fs3d_ctx *ctx, float *ms_out);

/* Solver3D::ClearOutterCells (Solver3D.cpp:41-44) = TimeLayer3D::Clear(grid, NODE_OUT, 0, 0, 0, (FTYPE)baseT) on one layer:
 * U, V, W := 0 and T := baseT on the NODE_OUT cells of the current geometry, every other cell untouched.  Needed once cells
 * change type: fs3d_get_layer stamps 99999 into the NODE_OUT cells of `next`, and a cell that becomes NODE_IN starts from
 * what its layer holds (unless fs3d_fill_fresh_cells above gives it the mean of its fluid neighbours). */
fs3d_status fs3d_clear_outer_cells(fs3d_ctx *ctx, int layer, double baseT);
/* Device time of the last fs3d_update_nodes* call: its kernels and copies on the context's stream, summed over HIP event pairs
 * around every batch of launches (the host's decisions between the batches are not in it).  Measured while fs3d_enable_timing is
 * on, else 0.  Measurement aid (tools/geometry_update_cost.py). */
fs3d_status fs3d_last_update_device_ms(fs3d_ctx *ctx, float *ms_out);
/* Summary of the geometry tables, the same after an upload and after an update of the same geometry.  info[0..2] segment
 * counts X, Y, Z; [3] BOUND / VALVE cells; [4] NODE_IN cells on no segment of some direction; [5..7] dead lines X, Y, Z;
 * [8..9] shared-column groups flagged uniform in X, Y; [10..11] distinct shared columns in X, Y; [12] an order-independent
 * 64-bit digest of the cell-code table (sum over cells of a mix of cell index and code), computed on the device from the
 * table the sweeps read; [13] the number of device allocations and frees fs3d_upload_nodes / fs3d_update_nodes* / fs3d_fill_fresh_cells* and the accumulators of FS3D_OPT_TIME_STATS (the cross sums of FS3D_OPT_TIME_STATS_CROSS the gradient sums of FS3D_OPT_TIME_STATS_GRAD and the wall sums of FS3D_OPT_TIME_STATS_WALL among them) have made
 * since the context was created (the one entry that describes the path taken, not the tables).
 * Measurement and test aid; no reference counterpart. */
#define FS3D_N_GEOM_INFO 14
fs3d_status fs3d_geometry_info(fs3d_ctx *ctx, long long info[FS3D_N_GEOM_INFO]);
/* Test and measurement aid, for any context with a geometry: the dead-line bytes of direction dir (0 X: [j][k], 1 Y: [i][k],
 * 2 Z: [i][j], i over the context's own planes) -- 1 where no cell of the context's piece of the line is NODE_IN or on a segment.
 * fs3d_geometry_info counts them; which lines they are is what a slab update has to get right for X, where the piece is not the
 * line.  n_lines_out (may be NULL) receives the number of lines; dead_out (may be NULL: the count alone) that many bytes. */
fs3d_status fs3d_geometry_dead_lines(fs3d_ctx *ctx, int dir, uint8_t *dead_out, long long *n_lines_out);

/* ---- layers -----------------------------------------------------------------
 * TimeLayer3D(backend, grid) constructor: cur <- every node's v and T
 * (TimeLayer3D.h:736-780 CopyFromGrid, :1076-1090); other layers zero. */
fs3d_status fs3d_init_layers_from_nodes(fs3d_ctx *ctx);
/* multiDevMemcpy H2D / D2H of one layer's four fields (GPUplan.h:110-179,
 * TimeLayer3D::CopyLayerTo, TimeLayer3D.h:685-724).  NULL pointers are skipped. */
fs3d_status fs3d_upload_layer(fs3d_ctx *ctx, int layer, const void *u, const void *v,
                              const void *w, const void *T);
fs3d_status fs3d_download_layer(fs3d_ctx *ctx, int layer, void *u, void *v, void *w, void *T);
/* device pointer of one field (owned planes only), for zero-copy interop
 * (ScalarField3D::getMultiArray, TimeLayer3D.h:267-270). */
fs3d_status fs3d_field_dev_ptr(fs3d_ctx *ctx, int layer, int var, void **dev_ptr);

/* ---- the hot path -------------------------------------------------------------
 * AdiSolver3D::UpdateBoundaries (AdiSolver3D.cpp:286-304): re-impose NODE_BOUND and
 * NODE_VALVE node values into cur (CPU semantics: CopyFromGrid of both types). */
fs3d_status fs3d_update_boundaries(fs3d_ctx *ctx);

/* AdiSolver3D::TimeStep (AdiSolver3D.cpp:306-391) with CPU-backend ordering (all
 * four variables of a sweep read the same temp; merge after the sweep).
 * compute_error != 0 evaluates EvalDivError on next; *err_out (optional) receives the
 * solver's diffError member (last evaluated value).  Returns FS3D_ERR_DIVERGED, and
 * does NOT swap cur/next, when diffError > 0.01 -- where the reference throws. */
fs3d_status fs3d_time_step(fs3d_ctx *ctx, double dt, int num_global, int num_local,
                           int compute_error, double *err_out);

/* Asynchronous variant used by the benchmark loop: enqueues the step on the
 * context's stream and returns; no divergence check, no host sync.  Call
 * fs3d_synchronize() before reading results. */
fs3d_status fs3d_time_step_async(fs3d_ctx *ctx, double dt, int num_global, int num_local);
fs3d_status fs3d_synchronize(fs3d_ctx *ctx);

/* One sweep = one pass of SolveSegments_GPU (AdiSolver3D.h:40-41; CPU semantics of
 * AdiSolver3D.cpp:593-603) over every segment of `dir`: reads layers l_cur and l_temp,
 * writes l_next.  merge_into_temp != 0 also performs the following
 * next->MergeLayerTo(grid, temp, NODE_IN) (AdiSolver3D.cpp:651).  Exposed for
 * kernel-level parity tests and profiling. */
fs3d_status fs3d_sweep(fs3d_ctx *ctx, int dir, double dt, int l_cur, int l_temp, int l_next,
                       int merge_into_temp);
/* TimeLayer3D::MergeLayerTo(grid, dest, NODE_IN), TimeLayer3D.h:664-683 / MergeFieldTo_GPU */
fs3d_status fs3d_merge(fs3d_ctx *ctx, int l_src, int l_dest);
/* TimeLayer3D::EvalDivError (TimeLayer3D.h:595-641): mean |div| over NODE_IN cells.
 * count_out (optional) receives the number of cells summed.  In a multi-GPU group the
 * sum and count are all-reduced (the reference's MPI_Reduce+Bcast, :630-637): the per-workgroup sums of all
 * global planes are gathered and added in the order a single context of the global grid adds them, so every
 * rank reports what that context would report from the same fields, bit for bit. */
fs3d_status fs3d_eval_div_error(fs3d_ctx *ctx, int layer, double *err_out, long long *count_out);

/* Solver3D::GetLayer (Solver3D.cpp:21-25): next->Clear(NODE_OUT -> MISSING_VALUE 99999)
 * then FilterToArrays (TimeLayer3D.h:819-924): nearest-neighbour down-sample into
 * outV (Vec3D[] = interleaved real x,y,z) and outT (double[]).  outdim == 0 means the
 * layer's own dim.  Reads `next`, which after the swap in TimeStep is the previous
 * step's layer -- the reference's one-step output lag is preserved. */
fs3d_status fs3d_get_layer(fs3d_ctx *ctx, void *outV, double *outT,
                           int outdimx, int outdimy, int outdimz);
/* The same output (Solver3D.cpp:21-25, TimeLayer3D.h:819-924) for an x-slab of a GLOBAL result: outV / outT are the arrays of
 * the WHOLE output grid (outdimx*outdimy*outdimz samples, 0 = the GLOBAL dim), and the context writes the rows i whose source
 * plane i*dimx_global/outdimx it owns -- rows[0] = ceil(x_offset*outdimx/dimx_global) up to
 * rows[1] = ceil((x_offset+dimx)*outdimx/dimx_global), reported in `rows`.  Over the slabs of a group the ranges partition
 * [0, outdimx) in rank order; a slab that owns no row writes nothing and returns FS3D_OK; a single context writes everything.
 * (fs3d_get_layer on a slab samples the slab's OWN planes, x = i*dimx/outdimx, as it always did.)
 * The samples are gathered by a kernel, one thread per sample, behind the 99999 stamp on the same stream: only the owned samples
 * cross the bus, (rows[1]-rows[0])*outdimy*outdimz*(3*sizeof(real)+8) bytes, through a device staging buffer the context keeps
 * and only grows.  Host destinations; returns synchronised.
 * All three entries stamp `next` first and over all owned cells, refuse before any launch (NULL context, destination or rows,
 * negative dims, no nodes yet: FS3D_ERR_INVALID, the context stays usable) and report pending device errors.
 *
 * Filtered and derived records (FS3D_OPT_OUTPUT_FILTER, FS3D_OPT_OUTPUT_VECTOR, FS3D_OPT_OUTPUT_GRADIENT, FS3D_OPT_OUTPUT_WALL; no reference counterpart; the rule and its numpy
 * twin: cmc_fluid_solver_amd/layer_output.py).  With either option non-zero the three entries run k_get_layer_box
 * (csrc/kernels_output.hip) in place of the gather, behind the same stamp, through the same staging buffer and copies: `next` is left as a default call leaves it.
 * The box of output index i on an axis of g source cells and o samples is [lo, hi), lo = i*g/o, hi = max(lo + 1, (i+1)*g/o) in
 * 64-bit integers: for o <= g the boxes partition the axis and start at the reference's sample cell, for o >= g each is that cell.
 * Per cell q = (a, b, c, T): (a, b, c) is the velocity, or with FS3D_OPT_OUTPUT_VECTOR set to 1 the vorticity in the context's real
 * type R, each operation rounded, two_dx = R(2) * R(dx):
 *   wx = (W[j+1] - W[j-1]) / two_dy - (V[k+1] - V[k-1]) / two_dz
 *   wy = (U[k+1] - U[k-1]) / two_dz - (W[i+1] - W[i-1]) / two_dx
 *   wz = (V[i+1] - V[i-1]) / two_dx - (U[j+1] - U[j-1]) / two_dy
 * on a NODE_IN cell whose six neighbours are inside the grid and not NODE_OUT (their fields hold the stamp); (99999, 99999, 99999)
 * on a NODE_OUT cell; (0, 0, 0) on every other cell.  With FS3D_OPT_OUTPUT_GRADIENT set to 1 (a, b, c) is (div, Q, SS), the
 * invariants of the velocity gradient, on the same cells and with the same values elsewhere.  With a over the fields U, V, W
 * (indices x, y, z), b over the axes and h = R(0.5), every operation rounded once in R, in this order, nothing fused:
 *   g_ab = (u_a[b+1] - u_a[b-1]) / two_db                                   nine quotients
 *   div  = (g_xx + g_yy) + g_zz
 *   s_xy = h*(g_xy + g_yx)   s_xz = h*(g_xz + g_zx)   s_yz = h*(g_yz + g_zy)
 *   o_xy = h*(g_xy - g_yx)   o_xz = h*(g_xz - g_zx)   o_yz = h*(g_yz - g_zy)
 *   SS   = ((g_xx*g_xx + g_yy*g_yy) + g_zz*g_zz) + R(2)*((s_xy*s_xy + s_xz*s_xz) + s_yz*s_yz)      S:S (2 nu S:S is the dissipation)
 *   OO   = R(2)*((o_xy*o_xy + o_xz*o_xz) + o_yz*o_yz)
 *   Q    = h*(OO - SS)                                                                              positive inside a vortex
 * Everything said of the vector option below holds for FS3D_OPT_OUTPUT_GRADIENT 1 as well: the slab refusals, and with
 * FS3D_OPT_OUTPUT_SLABS the same collective call with the same one ghost plane and type plane per neighbour.  The two options
 * exclude each other: with both non-zero the three entries return FS3D_ERR_INVALID before any launch.
 * Wall loads (FS3D_OPT_OUTPUT_WALL 1 and 2; whole-grid contexts only; the rule: layer_output.wall_loads).  A wall cell B (NODE_BOUND
 * or NODE_VALVE) has the exposed face (d, s), axis d and s = -1 or +1, iff P = B + s*e_d is inside the grid, NODE_IN and an INTERIOR
 * row of direction d of the geometry tables (its index along the line is >= 1 and a cell that is not NODE_IN lies beyond it): the
 * faces where the solver imposes B's node value on the line through P.  A carrier is a wall cell with at least one exposed face.
 * With A_x = R(dy)*R(dz), A_y = R(dx)*R(dz), A_z = R(dx)*R(dy), h_d = R(d_d), nu = R(v_vis), kappa = R(t_vis) of fs3d_set_params,
 * all sums from R(0), the exposed faces in the order x-, x+, y-, y+, z-, z+, every operation rounded once in R, nothing fused:
 *   area = area + A_d
 *   velocity BC of B NOSLIP, each component c != d:   g = (F_c[P] - F_c[B]) / h_d ;  t = nu * g ;     sum_c = sum_c + A_d * t
 *   temperature BC of B NOSLIP:                       g = (T[P] - T[B]) / h_d ;      t = kappa * g ;  sum_q = sum_q + A_d * t
 *   tau_c = sum_c / area     q = sum_q / area     mag = sqrt((tau_x*tau_x + tau_y*tau_y) + tau_z*tau_z)     (correctly rounded)
 * tau is the shear traction the fluid exerts on the wall (fluid moving +x over a wall at rest gives tau_x > 0 on either side of the
 * wall; the wall-normal component of a face's own axis is left out), q > 0 is heat flowing into the wall.  A FREE face adds its
 * area and nothing else: an outflow face is a carrier with zero loads.  F[B] is read from the sampled layer, so a wall that carries
 * a velocity gives the relative shear.  (a, b, c) is tau (value 1) or (mag, q, area) (value 2) on the carriers, 99999 on NODE_OUT
 * cells, 0 on every other cell.  For these two values the C of filter 1 below is the carriers of the box, not its NODE_IN cells.
 * Not provided: x-slabs; second-order one-sided differences; the wall-normal viscous stress and any pressure-like force.
 * Filter 0: the sample is q of the cell (lo_x, lo_y, lo_z).  Filter 1: with C
 * the NODE_IN cells of the sample's box, the sample is filter 0's where C is empty (a wall value or 99999: walls and the outside
 * show only where a box holds no fluid); else each quantity is m = (sum over C of (double)q) / (double)|C|, summed in double in an
 * unspecified order, one double division; outT = m, each outV component is m rounded once to R.  With every o >= g filter 1 equals
 * filter 0 bit for bit; a field that is constant on NODE_IN comes out as that constant wherever |C| times it is exact in double
 * (in fp32: every box of up to 2^29 cells).
 * While either option is non-zero, an x-slab (x_offset != 0 or dimx != dimx_global) or a member of a group is refused by all three
 * entries with FS3D_ERR_UNSUPPORTED before any launch, destinations and `next` untouched: a box can straddle a cut and the curl
 * needs the neighbour's planes.  fs3d_get_layer_rows / _dev on a whole-grid context work and report rows = [0, outdimx).
 *
 * On x-slabs (FS3D_OPT_OUTPUT_SLABS set to 1 on every member of a group): fs3d_get_layer_rows and fs3d_get_layer_dev, with either
 * option non-zero, as one COLLECTIVE call.  The rows a slab writes are the rows [ceil(x_offset*odx/gx), ceil((x_offset+dimx)*odx/gx))
 * of the record a single context of the GLOBAL grid writes -- the rule above applied to the global types and fields; over the ranks
 * they partition [0, odx) as ever.  The vorticity of an own cell tests the GLOBAL x against the grid's faces and takes the x
 * neighbours across a cut from the neighbour's stamped boundary plane and node types: its bits are the single context's, so with
 * filter 0 the rows equal the global record bit for bit.  Box mean: every slab sums (double)q and counts over the NODE_IN cells of
 * the box that lie in its own planes; for a row whose box holds planes of more than one slab (at most nranks - 1 rows, whatever the
 * width of a box) the slabs' sums and counts are added over the group (the counts exactly, as doubles below 2^53), then one division
 * and one rounding as above, by the slab that holds the first plane of the box; a box without a NODE_IN cell on any slab gives the
 * point sample of (lo_x, lo_y, lo_z), which that slab holds.  The rule leaves the order of the double sum free: the bound of a
 * single context's record holds, and wherever the sums are exact the rows equal it bit for bit.  FS3D_OPT_OUTPUT_SOURCE and
 * FS3D_OPT_OUTPUT_MOMENT combine as on one GPU; the statistic layer Q then has a ghost plane on either side.
 * What runs, on every rank alike whatever it owns (a rank without a row takes part to the end): all refusals; the statistic layer
 * and the stamp on the own cells; with the vector option ONE grouped exchange per neighbour -- the boundary plane of the four fields
 * of the sampled layer and one plane of node types, a byte per cell, derived from the current geometry per call; the slab kernel,
 * which finishes the rows inside the slab and leaves five doubles per sample of a straddling row; ONE all-reduce of those partial
 * sums, at most (nranks - 1) * ody * odz * 40 bytes, skipped when no row straddles a cut (every rank finds the same list from the
 * cuts of the group, which are gathered once per context); the finishing kernel on the row's owner; staging, copies, rows and
 * fs3d_get_layer_info as ever.  No source plane beyond that one ghost plane travels.
 * The contract, as for the collective fresh-cell fill: every rank makes the call between the same two steps, with the same output
 * dims, the same filter, vector, source and moment options, and FS3D_OPT_OUTPUT_SLABS at 1.  A rank that fails inside the call
 * aborts the group's transport (fs3d_comm_abort): its peers return FS3D_ERR_COMM instead of waiting.  fs3d_get_layer_dev may
 * synchronise inside the call in this mode (the in-process transport does).  `next` and `cur` are left as a default call leaves
 * them, but with the vector option the ghost planes of the sampled layer are overwritten (every time step exchanges them again).
 * The type planes, the partial sums, the cuts and a Q with ghost planes are allocated by the first call that needs them, kept and
 * only grown, and counted in fs3d_get_layer_info entry 2: nothing is allocated in steady state.
 * Still refused with FS3D_ERR_UNSUPPORTED, before any launch and any word to a peer, destinations, rows and layers untouched: a lone
 * slab of a larger grid in no group, and fs3d_get_layer on any slab.  The FS3D_ERR_INVALID refusals of the time statistics come
 * before any exchange too.  Between devices and over RCCL the path is compiled and has not been run.
 *
 * Time statistics (FS3D_OPT_TIME_STATS, FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_TIME_STATS_EVERY, FS3D_OPT_TIME_STATS_GRAD, FS3D_OPT_TIME_STATS_WALL,
 * FS3D_OPT_OUTPUT_SOURCE, FS3D_OPT_OUTPUT_MOMENT, FS3D_OPT_OUTPUT_GRADIENT 2, FS3D_OPT_OUTPUT_WALL 3 and 4; no reference counterpart; the rule and its numpy twin: cmc_fluid_solver_amd/time_stats.py).  While
 * FS3D_OPT_TIME_STATS is 1 or 2, every fs3d_time_step that returns FS3D_OK and every fs3d_time_step_async is a CANDIDATE step of the
 * open window, counted s = 1, 2, ..; a step that returns FS3D_ERR_DIVERGED does not swap and is no candidate.  With k the value of
 * FS3D_OPT_TIME_STATS_EVERY (default 1), candidate s is ACCUMULATED if and only if (s - 1) % k is 0: the first step of a window always
 * counts, so a window of at least one step is never empty, and on the other steps no kernel runs.  An accumulated step enqueues one
 * kernel behind the step, after the cur / next swap, over the context's own cells: for each cell that is NODE_IN in the geometry of
 * that moment, with x each of U, V, W, T of FS3D_LAYER_CUR,
 *   n += 1 (uint32 per cell),  S1 += (double)x,  in mode 2  S2 += (double)x * (double)x,
 *   and in mode 2 with FS3D_OPT_TIME_STATS_CROSS set to 1  S_ab += (double)x_a * (double)x_b  for the six pairs
 *   0 uv, 1 uw, 2 vw, 3 uT, 4 vT, 5 wT
 * -- the product rounded once, the addition rounded once, in double, no fused multiply-add -- and the window's step count N grows by
 * one: N and the per-cell n count accumulated steps only, and the fluid fraction stays n / N.  The geometry may change inside a
 * window (fs3d_update_nodes*, fs3d_upload_nodes): a cell is counted by the type it has at each accumulated step, which is what the
 * per-cell n is for.  While the mode is 0 or 1 the CROSS option has no effect.
 *  - gradient sums (FS3D_OPT_TIME_STATS_GRAD set to 1, whole-grid contexts only): every accumulated step enqueues one more kernel
 *    behind the one above, over the context's own cells.  On each cell that carries invariants in the geometry of that moment
 *    (NODE_IN, the six neighbours inside the grid and not NODE_OUT), with (div, Q, SS) the R values of the GetLayer section's rule
 *    on FS3D_LAYER_CUR after the swap:  ng += 1 (uint32),  G_div += (double)div,  G_Q += (double)Q,  G_SS += (double)SS,  each
 *    addition rounded once in double.  The invariants are quadratic in the gradient, so their time mean cannot be had from the
 *    mean field.  28 bytes per own cell in two buffers (the counts; the three sums), allocated by the first accumulation that
 *    needs them, kept over windows, counted in fs3d_geometry_info entry 13, freed by setting this option or FS3D_OPT_TIME_STATS
 *    to 0 (after a stream synchronise) and by fs3d_destroy.  The refusals on slabs and group members: the option's entry above.
 *    Read-out, FS3D_OPT_OUTPUT_GRADIENT 2 with FS3D_OPT_OUTPUT_SOURCE 1: the statistic layer is
 *      Q_U, Q_V, Q_W = (R)(G_div / (double)ng), (R)(G_Q / (double)ng), (R)(G_SS / (double)ng)  where ng >= 1, R(0) where ng = 0,
 *      Q_T = source 1's (the mean of T, or `cur` where n = 0),
 *    and the call then runs unchanged on Q as a velocity layer: the stamp on the cells that are NODE_OUT now, the gather or the
 *    box mean, staging, copies, rows, fs3d_get_layer_info.  Refused with FS3D_ERR_INVALID before any launch, destinations, rows
 *    and layers untouched: a source other than 1, FS3D_OPT_TIME_STATS at 0, FS3D_OPT_TIME_STATS_GRAD at 0 in the open window, a
 *    window without an accumulated step, and FS3D_OPT_OUTPUT_VECTOR 1.
 *  - wall sums (FS3D_OPT_TIME_STATS_WALL set to 1, whole-grid contexts only): every accumulated step enqueues one more kernel,
 *    k_time_wall, behind the ones above.  On each carrier of the geometry of that moment, with tau, mag and q the R values of the
 *    GetLayer section's wall rule on FS3D_LAYER_CUR after the swap:  nw += 1 (uint32),  W_x, W_y, W_z += (double)tau_c,
 *    W_mag += (double)mag,  W_q += (double)q,  each addition rounded once in double.  The mean of |tau| (TAWSS) and the oscillatory
 *    shear index cannot be had from the mean field.  44 bytes per own cell in two buffers (the counts; the five sums), allocated by
 *    the first accumulation that needs them, kept over windows, counted in fs3d_geometry_info entry 13, freed by setting this
 *    option or FS3D_OPT_TIME_STATS to 0 (after a stream synchronise) and by fs3d_destroy.  Read-out, FS3D_OPT_OUTPUT_WALL 3 or 4
 *    with FS3D_OPT_OUTPUT_SOURCE 1: the statistic layer is, in double with dn = (double)nw where nw >= 1,
 *      3:  Q_U, Q_V, Q_W = (R)(W_x / dn), (R)(W_y / dn), (R)(W_z / dn)
 *      4:  m_c = W_c / dn ;  mm = sqrt((m_x*m_x + m_y*m_y) + m_z*m_z) ;  tawss = W_mag / dn
 *          osi = tawss > 0 ? 0.5 * (1 - mm / tawss) : 0, 0 where that is negative
 *          Q_U, Q_V, Q_W = (R)tawss, (R)(W_q / dn), (R)osi
 *    and R(0) where nw = 0; Q_T is source 1's.  The call then runs unchanged on Q as a velocity layer; with filter 1 C is the cells
 *    of the box with nw >= 1 that are not NODE_OUT now.  Refused with FS3D_ERR_INVALID before any launch: a source other than 1,
 *    FS3D_OPT_TIME_STATS at 0, FS3D_OPT_TIME_STATS_WALL at 0 in the open window, a window without an accumulated step.
 *  - the window: every fs3d_set_option of FS3D_OPT_TIME_STATS, FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_TIME_STATS_EVERY,
 *    FS3D_OPT_TIME_STATS_GRAD or FS3D_OPT_TIME_STATS_WALL opens a new
 *    one, N = 0, no candidate yet and all sums zero, whatever the value was.
 *  - memory: 4 + 32 (mode 2: 64; with the cross sums: 112) bytes per own cell, no ghost planes.  Each buffer is allocated by the first
 *    accumulation that needs it (a failed allocation is that step's status: the step itself stands, nothing was accumulated), kept
 *    over later windows, and counted in fs3d_geometry_info entry 13: mode 2 makes 3 allocations, with the cross sums 4.  Setting
 *    FS3D_OPT_TIME_STATS to 0 frees all of them, setting FS3D_OPT_TIME_STATS_CROSS to 0 the cross sums, either after a stream
 *    synchronise; fs3d_destroy frees what is left.  With FS3D_OPT_TIME_STATS at 0 nothing is allocated and no kernel runs; the stride
 *    needs no memory.
 *  - read-out: with FS3D_OPT_OUTPUT_SOURCE 1..3 the three GetLayer entries first build a statistic layer Q -- four fields of the
 *    context's real type R in a buffer of the context's own (4 fields of the own cells, allocated by the first such call, counted
 *    in fs3d_get_layer_info entry 2, kept) -- and then run on Q what they run on `next`.  Per cell with n >= 1, dn = (double)n and
 *    m_a = S1_a / dn:
 *      1 time mean       Q = (R)m
 *      2 second moments, chosen by FS3D_OPT_OUTPUT_MOMENT (read for this source only):
 *        moment 0  the variances: var_a = S2_a / dn - m_a * m_a, 0 where that is negative, Q = (R)var   (the population variance
 *                  over the n steps)
 *        moment 1  the Reynolds stresses: cov(a,b) = S_ab / dn - m_a * m_b, NOT clamped (a covariance may be negative);
 *                  Q_U = (R)cov(u,v), Q_V = (R)cov(u,w), Q_W = (R)cov(v,w), Q_T = (R)(0.5 * ((var_u + var_v) + var_w)), the
 *                  turbulent kinetic energy, from the clamped variances of moment 0
 *        moment 2  the turbulent heat flux: Q_U = (R)cov(u,T), Q_V = (R)cov(v,T), Q_W = (R)cov(w,T), Q_T = (R)var_T
 *      3 fluid fraction  Q_T = (R)((double)n / (double)N), Q_U = Q_V = Q_W = 0
 *    all in double, each operation rounded once; with n = 0: source 1 the value the cell holds in FS3D_LAYER_CUR (walls show their
 *    node values as in every record), sources 2 (every moment) and 3 zero.  Then, unchanged: the 99999 stamp on the cells that are
 *    NODE_OUT in the CURRENT geometry (written into Q), the gather -- or with FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR the box
 *    mean of the layer and, for the mean and the variances, the curl --, staging, copies, rows and the fs3d_get_layer_info counts.
 *    outT is the widening of Q_T.  `next` and `cur` are not written.  The one-pass variance and covariance cancel where the means
 *    are large against the fluctuation (absolute error about 2 * 2^-53 * |m_a * m_b|).
 *  - refusals, FS3D_ERR_INVALID before any launch with the destinations, rows and layers untouched: a source the current
 *    FS3D_OPT_TIME_STATS mode does not hold (any source at 0, source 2 at 1); source 2 with moment 1 or 2 while the open window holds
 *    no cross sums (FS3D_OPT_TIME_STATS_CROSS is 0, or the mode is below 2); moment 1 or 2 with source 2 and FS3D_OPT_OUTPUT_VECTOR 1
 *    (the curl of a stress layer means nothing) or FS3D_OPT_OUTPUT_GRADIENT 1; and a window without an accumulated step (N = 0).  The slab refusal of the filter
 *    and vector options stands while FS3D_OPT_OUTPUT_SLABS is 0; without them an x-slab or group member accumulates and reads out
 *    its own planes -- every layer is per cell --, and the rows the slabs write are those of the global record a single context
 *    gives.  With FS3D_OPT_OUTPUT_SLABS at 1 on a group every source combines with the filter and the curl as on one GPU, as the
 *    collective call described above; Q then carries a ghost plane on either side (two more planes per field), and the refusals of
 *    this list come before any exchange.
 *  - not provided: third moments; covariances with the vorticity; second moments of the invariants; gradient sums on x-slabs (they
 *    need an exchange of the ghost planes of `cur` per accumulated step, a collective of their own); wall sums on x-slabs and on a
 *    compact list of wall cells; lambda_2, the eigenvalues
 *    and the nine components of the gradient; a history of the cells that are NODE_OUT now (they are stamped
 *    as in every record); the 2D solver. */
fs3d_status fs3d_get_layer_rows(fs3d_ctx *ctx, void *outV, double *outT, int outdimx, int outdimy, int outdimz, int rows[2]);
/* fs3d_get_layer_rows (Solver3D.cpp:21-25, TimeLayer3D.h:819-924) with the two arrays on the context's DEVICE: the kernel
 * writes them directly, nothing is copied.  Returns after the enqueue on the context's stream; read after fs3d_synchronize.
 * (As the collective call of FS3D_OPT_OUTPUT_SLABS it may synchronise inside the call; read after fs3d_synchronize all the same.)
 * The zero-copy partner of fs3d_field_dev_ptr and fs3d_update_nodes_dev. */
fs3d_status fs3d_get_layer_dev(fs3d_ctx *ctx, void *outV_dev, double *outT_dev, int outdimx, int outdimy, int outdimz, int rows[2]);
/* What the result output (Solver3D.cpp:21-25, TimeLayer3D.h:819-924) did: info[0] samples the last fs3d_get_layer* call wrote,
 * [1] bytes it copied device-to-host, [2] device allocations the get-layer calls have made since fs3d_create.
 * Measurement and test aid; no reference counterpart. */
#define FS3D_N_GETLAYER_INFO 3
fs3d_status fs3d_get_layer_info(fs3d_ctx *ctx, long long info[FS3D_N_GETLAYER_INFO]);

/* ---- multi-GPU (one process per GPU, x-slabs) ---------------------------------
 * Replaces GPUplan peer copies / PARAplan MPI point-to-point (TimeLayer3D.h:47-247,
 * 272-335) with RCCL.  unique_id is the 128-byte ncclUniqueId produced by
 * fs3d_comm_unique_id() on rank 0 and broadcast by the caller (e.g. torch.distributed). */
fs3d_status fs3d_comm_unique_id(void *unique_id_128);
fs3d_status fs3d_comm_init(fs3d_ctx *ctx, const void *unique_id_128, int rank, int nranks);

/* The reference's other multi-GPU mode: ONE process driving several GPUs (GPUplan, Common/GPUplan.h:29-108,
 * `multiDev*` helpers).  Here: one slab context per GPU, each driven by its own host thread, joined by an
 * in-process group -- halos and carries move as device-to-device copies with a host rendezvous instead of
 * RCCL.  Every collective call (time_step, sweep, eval_div_error ...) must then be made by all the
 * group's threads concurrently, as with RCCL ranks.  Contexts may share a device (used to exercise the
 * slab protocol on a single card).  Destroy the contexts before the group. */
fs3d_status fs3d_local_group_create(int nranks, void **group_out);
void fs3d_local_group_destroy(void *group);
/* a driver thread that fails before it holds a context (Init threw) releases the others: every member's pending and later
 * exchange returns FS3D_ERR_COMM */
void fs3d_local_group_abort(void *group);
fs3d_status fs3d_comm_init_local(fs3d_ctx *ctx, void *group, int rank);
/* A rank / slab thread that cannot go on (its own call failed, its driver thread threw) takes the group down: the peers'
 * pending and later exchanges return FS3D_ERR_COMM instead of blocking (the reference: gpuSafeCall / mpiSafeCall throw,
 * main catches and calls MPI_Abort, GPUplan.cpp:173-193, FluidSolver3D.cpp:272-283).  The library calls it itself when a
 * multi-step exchange (the cross-slab X sweep) fails half way. */
fs3d_status fs3d_comm_abort(fs3d_ctx *ctx);
/* Wire check on one card: a communicator of ONE rank is created on the context's device and the three RCCL shapes the slab
 * protocol uses are run and verified -- a grouped ncclSend/ncclRecv pair (the halo-plane / carry-row shape, to the own rank,
 * on the exchange stream), ncclAllGather (the interface words of the cross-slab X solve) and the 2-double ncclAllReduce of
 * EvalDivError.  Says whether librccl loads, initialises and moves bytes inside this library (beside the caller's own RCCL);
 * it does not replace a run on several GPUs.  `elems` elements of the context's precision per message. */
fs3d_status fs3d_comm_selftest(fs3d_ctx *ctx, size_t elems);

/* ---- measurement ---------------------------------------------------------------
 * Wall time of the kernels of the last fs3d_time_step* call, measured with HIP events
 * on the context's stream: ms[0]=Z sweeps, [1]=Y sweeps, [2]=X sweeps, [3]=everything
 * else; n[] = number of launches in each class.  Profiler.h event names map onto these. */
fs3d_status fs3d_last_step_timing(fs3d_ctx *ctx, float ms[4], int n[4]);
/* The same device times under the event names of the reference's Profiler (Common/Profiler.h:44-134; StartEvent/StopEvent
 * sites AdiSolver3D.cpp:297-367, 555-680): SolveSegments_Z/_Y/_X, CopyLayer, MergeLayer (zero launches while the merge is fused
 * into the sweeps), EvalDivError, UpdateBoundaries, syncHalos, CreateSegments (host time of fs3d_upload_nodes and fs3d_update_nodes*, one launch per call that succeeded).  names[] receives
 * static strings.  The driver prints them as the reference's PrintTimings table. */
#define FS3D_N_EVENTS 9
fs3d_status fs3d_profiler_events(fs3d_ctx *ctx, const char *names[FS3D_N_EVENTS], float ms[FS3D_N_EVENTS], int n[FS3D_N_EVENTS]);
/* per-class event timing: 0 off (default), 1 two events around every launch, N > 1 the same on every N-th time step only
 * (a sample: the events themselves cost a few microseconds per launch) */
fs3d_status fs3d_enable_timing(fs3d_ctx *ctx, int on);

/* One pipelined sweep (merge fused, result discarded into the spare temp buffer) with
 * in-kernel time stamps: for each of the first *n_blocks_out (<= max_blocks) workgroups and
 * each of its 8 waves, 8 shader-clock stamps (start, rows built, relay turn begins, forward
 * done, backward begins, backward done, relay drained, stores issued).
 * stamps_out holds max_blocks*64 values.  Measurement aid; no reference counterpart. */
fs3d_status fs3d_profile_sweep(fs3d_ctx *ctx, int dir, double dt, int l_cur, int l_temp, int l_next,
                               unsigned long long *stamps_out, int max_blocks, int *n_blocks_out);

/* Which kernel the last sweep of direction dir (FS3D_DIR_*) really ran: FS3D_SWEEP_LINE / _PIPE / _PART, with
 * *segmented_out (optional): bit 0 = PIPE / LINE ran as halves through the HBM scratch (long lines, x-slabs); for dir X
 * of a multi-GPU group bits 1-2 = the cross-slab form that ran (1 pipelined, 2 reduced interface, 3 reduced interface with
 * the slab's interface words from a first pass of the partition kernel instead of the per-line walk).  0 = no sweep yet.
 * FS3D_SWEEP_AUTO never falls back silently: callers (bench.py, fs3d_run) print this. */
fs3d_status fs3d_last_sweep_kernel(fs3d_ctx *ctx, int dir, int *kernel_out, int *segmented_out);

/* Which partition kernel instance the last sweep of direction dir launched, and how.  pass 0: the sweep itself; pass 1: the
 * interface pass of a reduced-interface cross-slab X sweep.  out[0] is the family: 0 = that pass launched no partition kernel
 * (exact kernels, or the thread-per-line interface walk); 1 = k_sweep_part: {1, M, NCH, LT, XB, order, workgroups, 0};
 * 2 = k_sweep_part_z: {2, LPL, NW, LG, n_grp, workgroups, 0, 0}.  Cleared to family 0 when a sweep of that direction begins; a
 * sweep cut into plane ranges (halo overlap) leaves its last launch.  For tests that must prove which instance they ran. */
fs3d_status fs3d_last_sweep_launch(fs3d_ctx *ctx, int dir, int pass, int out[8]);

/* library / device identification */
const char *fs3d_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FS3D_H */
