// A recording stand-in for libfs3d_hip.so: the 31 entries of include/fs3d.h that host/fs3d_run.cpp links against, g++ only, no HIP and
// no GPU.  Test code (tests/test_host_driver_calls.py builds it as libfs3d_hip.so in a temporary directory); it ships in no build.
//   * every context keeps its own in-memory log, one line per call: the entry's name, its scalar arguments and a 64-bit FNV-1a hash of
//     every input array (lengths from the create dims, or from nvert / ntri).  A context is driven by one thread and no lock is shared
//     between contexts -- a shared lock would order the driver's threads and hide its races from ThreadSanitizer.
//     fs3d_destroy writes the log to $FS3D_STUB_LOG.<x_offset> (nothing without the variable).
//   * every output is a fixed function of the context's call history and never of how the grid is cut: n_seg_out is constant, the err
//     of fs3d_time_step depends on the step count, a sample of fs3d_get_layer / _rows on the record counter, the options set and the
//     GLOBAL sample index (the rows a context fills are those of the header's formula), the counters and timings are constants.
//   * FS3D_STUB_FAIL=<entry>:<x_offset>:<n>: the n-th call of that entry on that context returns FS3D_ERR_HIP with a text of its own.
//     Nothing else is injectable.
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../include/fs3d.h"

struct fs3d_ctx {
    int device, prec, dimx, dimy, dimz, x_offset, dimx_global;
    std::string log, err;
    std::map<int, int> options;
    std::map<std::string, int> calls;          // per entry, for the failure hook
    long steps = 0, records = 0;
    double last_err = 0;
    size_t cells() const { return (size_t)dimx_global * dimy * dimz; }
    size_t real() const { return prec == FS3D_F32 ? 4 : 8; }
};

namespace {
thread_local std::string create_error;

uint64_t fnv(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33; return x; }

void say(fs3d_ctx *c, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->log += buf;
    c->log += '\n';
}
std::string hashes(std::initializer_list<std::pair<const void *, size_t>> arrays)
{
    std::string s;
    char buf[24];
    for (auto &a : arrays) {
        if (a.first) std::snprintf(buf, sizeof buf, "%016" PRIx64, fnv(a.first, a.second)); else std::snprintf(buf, sizeof buf, "null");
        s += s.empty() ? "" : ",";
        s += buf;
    }
    return s;
}
// the failure hook; counts the call either way
bool fails(fs3d_ctx *c, const char *entry)
{
    const int n = ++c->calls[entry];
    const char *f = std::getenv("FS3D_STUB_FAIL");
    if (!f) return false;
    char name[64];
    int off = 0, nth = 0;
    if (std::sscanf(f, "%63[^:]:%d:%d", name, &off, &nth) != 3 || std::strcmp(name, entry) || off != c->x_offset || nth != n) return false;
    c->err = std::string("stub: ") + entry + " failed on the context at x_offset " + std::to_string(off) + ", call " + std::to_string(n);
    say(c, "%s FAILED", entry);
    return true;
}
#define ENTRY(name) do { if (!ctx) return FS3D_ERR_INVALID; if (fails(ctx, name)) return FS3D_ERR_HIP; } while (0)
void segs(int n_seg_out[3]) { if (n_seg_out) { n_seg_out[0] = 11; n_seg_out[1] = 22; n_seg_out[2] = 33; } }

fs3d_status nodes(fs3d_ctx *ctx, const char *name, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp, const void *vx,
                  const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    ENTRY(name);
    const size_t n = ctx->cells(), r = n * ctx->real();
    say(ctx, "%s %s", name, hashes({{type, n}, {bc_vel, n}, {bc_temp, n}, {vx, r}, {vy, r}, {vz, r}, {T, r}}).c_str());
    segs(n_seg_out);
    return FS3D_OK;
}
fs3d_status shape2d(fs3d_ctx *ctx, const char *name, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                    double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{
    ENTRY(name);
    const size_t n = (size_t)ctx->dimx_global * ctx->dimy;
    say(ctx, "%s dz=%.17g depth=%.17g depth_var=%.17g baseT=%.17g %s", name, dz, depth, depth_var, baseT,
        hashes({{cell2d, n}, {velx2d, 4 * n}, {vely2d, 4 * n}, {T2d, 4 * n}}).c_str());
    segs(n_seg_out);
    return FS3D_OK;
}
fs3d_status shape3d(fs3d_ctx *ctx, const char *name, const float *x, const float *y, const float *z, const float *wx, const float *wy,
                    const float *wz, bool vel, int nvert, const int *tri, int ntri, double baseT, double wallT, int n_seg_out[3])
{
    ENTRY(name);
    const size_t v = 4 * (size_t)nvert, t = 12 * (size_t)ntri;
    if (vel) say(ctx, "%s nvert=%d ntri=%d baseT=%.17g wallT=%.17g %s", name, nvert, ntri, baseT, wallT,
                 hashes({{x, v}, {y, v}, {z, v}, {wx, v}, {wy, v}, {wz, v}, {tri, t}}).c_str());
    else say(ctx, "%s nvert=%d ntri=%d baseT=%.17g %s", name, nvert, ntri, baseT, hashes({{x, v}, {y, v}, {z, v}, {tri, t}}).c_str());
    segs(n_seg_out);
    return FS3D_OK;
}
// the record of a context: rows [rows[0], rows[1]) of the global output grid, by the formula of fs3d_get_layer_rows
fs3d_status layer(fs3d_ctx *ctx, const char *name, void *outV, double *outT, int ox, int oy, int oz, int rows[2], bool whole)
{
    ENTRY(name);
    if (!ox) ox = ctx->dimx_global;
    if (!oy) oy = ctx->dimy;
    if (!oz) oz = ctx->dimz;
    const long long g = ctx->dimx_global;
    const int r0 = whole ? 0 : (int)(((long long)ctx->x_offset * ox + g - 1) / g);
    const int r1 = whole ? ox : (int)(((long long)(ctx->x_offset + ctx->dimx) * ox + g - 1) / g);
    uint64_t key = mix((uint64_t)ctx->records);
    for (int opt : {FS3D_OPT_OUTPUT_FILTER, FS3D_OPT_OUTPUT_VECTOR, FS3D_OPT_OUTPUT_SOURCE, FS3D_OPT_OUTPUT_MOMENT})   // what shapes a record
        if (ctx->options.count(opt) && ctx->options[opt]) key = mix(key ^ ((uint64_t)opt << 32 | (uint32_t)ctx->options[opt]));
    for (size_t s = (size_t)r0 * oy * oz; s < (size_t)r1 * oy * oz; s++) {
        const uint64_t h = mix(key + s);
        for (int c = 0; c < 3; c++) {
            const double v = (double)((h >> (16 * c)) & 0xffff) / 65536.0 - 0.5;
            if (ctx->prec == FS3D_F32) ((float *)outV)[3 * s + c] = (float)v; else ((double *)outV)[3 * s + c] = v;
        }
        outT[s] = 1.0 + (double)(h >> 48) / 65536.0;
    }
    say(ctx, "%s out=%dx%dx%d rows=%d..%d record=%ld", name, ox, oy, oz, r0, r1, ctx->records);
    ctx->records++;
    if (rows) { rows[0] = r0; rows[1] = r1; }
    return FS3D_OK;
}
}  // namespace

extern "C" {

fs3d_status fs3d_create(fs3d_ctx **out, int device, fs3d_precision prec, int dimx, int dimy, int dimz, double dx, double dy, double dz,
                        int x_offset, int dimx_global)
{
    if (!out) { create_error = "stub: fs3d_create without a destination"; return FS3D_ERR_INVALID; }
    fs3d_ctx *ctx = new fs3d_ctx{device, (int)prec, dimx, dimy, dimz, x_offset, dimx_global};
    say(ctx, "fs3d_create device=%d prec=%d dims=%dx%dx%d d=%.17g,%.17g,%.17g x_offset=%d dimx_global=%d", device, (int)prec, dimx, dimy, dimz,
        dx, dy, dz, x_offset, dimx_global);
    if (fails(ctx, "fs3d_create")) { create_error = ctx->err; fs3d_destroy(ctx); return FS3D_ERR_HIP; }
    *out = ctx;
    return FS3D_OK;
}
void fs3d_destroy(fs3d_ctx *ctx)
{
    if (!ctx) return;
    say(ctx, "fs3d_destroy");
    if (const char *base = std::getenv("FS3D_STUB_LOG")) {
        const std::string path = std::string(base) + "." + std::to_string(ctx->x_offset);
        if (FILE *f = std::fopen(path.c_str(), "w")) { std::fwrite(ctx->log.data(), 1, ctx->log.size(), f); std::fclose(f); }
    }
    delete ctx;
}
const char *fs3d_last_error(const fs3d_ctx *ctx) { return ctx ? ctx->err.c_str() : create_error.c_str(); }

fs3d_status fs3d_set_params(fs3d_ctx *ctx, double v_T, double v_vis, double t_vis, double t_phi)
{
    ENTRY("fs3d_set_params");
    say(ctx, "fs3d_set_params %.17g %.17g %.17g %.17g", v_T, v_vis, t_vis, t_phi);
    return FS3D_OK;
}
fs3d_status fs3d_set_option(fs3d_ctx *ctx, int option, int value)
{
    ENTRY("fs3d_set_option");
    say(ctx, "fs3d_set_option %d %d", option, value);
    ctx->options[option] = value;
    return FS3D_OK;
}
fs3d_status fs3d_upload_nodes(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp, const void *vx,
                              const void *vy, const void *vz, const void *T, int n_seg_out[3])
{ return nodes(ctx, "fs3d_upload_nodes", type, bc_vel, bc_temp, vx, vy, vz, T, n_seg_out); }
fs3d_status fs3d_update_nodes(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp, const void *vx,
                              const void *vy, const void *vz, const void *T, int n_seg_out[3])
{ return nodes(ctx, "fs3d_update_nodes", type, bc_vel, bc_temp, vx, vy, vz, T, n_seg_out); }
fs3d_status fs3d_update_nodes_slab(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp, const void *vx,
                                   const void *vy, const void *vz, const void *T, int n_seg_out[3])
{ return nodes(ctx, "fs3d_update_nodes_slab", type, bc_vel, bc_temp, vx, vy, vz, T, n_seg_out); }
fs3d_status fs3d_update_nodes_shape2d(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                      double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{ return shape2d(ctx, "fs3d_update_nodes_shape2d", cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT, n_seg_out); }
fs3d_status fs3d_update_nodes_shape2d_slab(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                           double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{ return shape2d(ctx, "fs3d_update_nodes_shape2d_slab", cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT, n_seg_out); }
fs3d_status fs3d_update_nodes_shape3d(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert, const int *tri, int ntri,
                                      double baseT, int n_seg_out[3])
{ return shape3d(ctx, "fs3d_update_nodes_shape3d", x, y, z, nullptr, nullptr, nullptr, false, nvert, tri, ntri, baseT, 0, n_seg_out); }
fs3d_status fs3d_update_nodes_shape3d_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert, const int *tri,
                                           int ntri, double baseT, int n_seg_out[3])
{ return shape3d(ctx, "fs3d_update_nodes_shape3d_slab", x, y, z, nullptr, nullptr, nullptr, false, nvert, tri, ntri, baseT, 0, n_seg_out); }
fs3d_status fs3d_update_nodes_shape3d_vel(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx, const float *wy,
                                          const float *wz, int nvert, const int *tri, int ntri, double baseT, double wallT, int n_seg_out[3])
{ return shape3d(ctx, "fs3d_update_nodes_shape3d_vel", x, y, z, wx, wy, wz, true, nvert, tri, ntri, baseT, wallT, n_seg_out); }
fs3d_status fs3d_update_nodes_shape3d_vel_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                               const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                               double wallT, int n_seg_out[3])
{ return shape3d(ctx, "fs3d_update_nodes_shape3d_vel_slab", x, y, z, wx, wy, wz, true, nvert, tri, ntri, baseT, wallT, n_seg_out); }

fs3d_status fs3d_fill_fresh_cells(fs3d_ctx *ctx, int layer, int max_rounds, long long info[4])
{
    ENTRY("fs3d_fill_fresh_cells");
    say(ctx, "fs3d_fill_fresh_cells layer=%d max_rounds=%d", layer, max_rounds);
    if (info) { info[0] = 5; info[1] = 4; info[2] = 2; info[3] = 1; }
    return FS3D_OK;
}
fs3d_status fs3d_clear_outer_cells(fs3d_ctx *ctx, int layer, double baseT)
{
    ENTRY("fs3d_clear_outer_cells");
    say(ctx, "fs3d_clear_outer_cells layer=%d baseT=%.17g", layer, baseT);
    return FS3D_OK;
}
fs3d_status fs3d_init_layers_from_nodes(fs3d_ctx *ctx) { ENTRY("fs3d_init_layers_from_nodes"); say(ctx, "fs3d_init_layers_from_nodes"); return FS3D_OK; }
fs3d_status fs3d_update_boundaries(fs3d_ctx *ctx) { ENTRY("fs3d_update_boundaries"); say(ctx, "fs3d_update_boundaries"); return FS3D_OK; }
fs3d_status fs3d_time_step(fs3d_ctx *ctx, double dt, int num_global, int num_local, int compute_error, double *err_out)
{
    ENTRY("fs3d_time_step");
    say(ctx, "fs3d_time_step dt=%.17g global=%d local=%d error=%d", dt, num_global, num_local, compute_error);
    ctx->steps++;
    if (compute_error) ctx->last_err = 0.001 + 1e-5 * (double)(ctx->steps % 97);
    if (err_out) *err_out = ctx->last_err;
    return FS3D_OK;
}
fs3d_status fs3d_get_layer(fs3d_ctx *ctx, void *outV, double *outT, int outdimx, int outdimy, int outdimz)
{ return layer(ctx, "fs3d_get_layer", outV, outT, outdimx, outdimy, outdimz, nullptr, true); }
fs3d_status fs3d_get_layer_rows(fs3d_ctx *ctx, void *outV, double *outT, int outdimx, int outdimy, int outdimz, int rows[2])
{ return layer(ctx, "fs3d_get_layer_rows", outV, outT, outdimx, outdimy, outdimz, rows, false); }

fs3d_status fs3d_enable_timing(fs3d_ctx *ctx, int on) { ENTRY("fs3d_enable_timing"); say(ctx, "fs3d_enable_timing %d", on); return FS3D_OK; }
fs3d_status fs3d_profiler_events(fs3d_ctx *ctx, const char *names[FS3D_N_EVENTS], float ms[FS3D_N_EVENTS], int n[FS3D_N_EVENTS])
{
    ENTRY("fs3d_profiler_events");
    say(ctx, "fs3d_profiler_events");
    static const char *const event[FS3D_N_EVENTS] = {"SolveSegments_Z", "SolveSegments_Y", "SolveSegments_X", "CopyLayer", "MergeLayer",
                                                     "EvalDivError", "UpdateBoundaries", "syncHalos", "CreateSegments"};
    static const float total[FS3D_N_EVENTS] = {30.5f, 20.25f, 40.75f, 3.5f, 0.0f, 2.25f, 1.5f, 0.0f, 7.125f};   // distinct: the sort order is pinned
    static const int count[FS3D_N_EVENTS] = {24, 24, 24, 12, 0, 2, 12, 0, 1};
    for (int e = 0; e < FS3D_N_EVENTS; e++) { names[e] = event[e]; ms[e] = total[e]; n[e] = count[e]; }
    return FS3D_OK;
}
fs3d_status fs3d_last_sweep_kernel(fs3d_ctx *ctx, int dir, int *kernel_out, int *segmented_out)
{
    ENTRY("fs3d_last_sweep_kernel");
    say(ctx, "fs3d_last_sweep_kernel %d", dir);
    if (kernel_out) *kernel_out = dir == FS3D_DIR_Z ? FS3D_SWEEP_PIPE : FS3D_SWEEP_PART;
    if (segmented_out) *segmented_out = 0;
    return FS3D_OK;
}
fs3d_status fs3d_last_update_device_ms(fs3d_ctx *ctx, float *ms_out)
{
    ENTRY("fs3d_last_update_device_ms");
    say(ctx, "fs3d_last_update_device_ms");
    if (ms_out) *ms_out = 0.5f;
    return FS3D_OK;
}
fs3d_status fs3d_mesh_fill_rounds(fs3d_ctx *ctx, int *rounds_out)
{
    ENTRY("fs3d_mesh_fill_rounds");
    say(ctx, "fs3d_mesh_fill_rounds");
    if (rounds_out) *rounds_out = 3;
    return FS3D_OK;
}
fs3d_status fs3d_synchronize(fs3d_ctx *ctx) { ENTRY("fs3d_synchronize"); say(ctx, "fs3d_synchronize"); return FS3D_OK; }

// the group is a token: the stub's contexts exchange nothing, so there is nothing to rendezvous on or to abort
fs3d_status fs3d_local_group_create(int nranks, void **group_out)
{
    if (nranks < 1 || !group_out) return FS3D_ERR_INVALID;
    *group_out = new int(nranks);
    return FS3D_OK;
}
void fs3d_local_group_destroy(void *group) { delete (int *)group; }
void fs3d_local_group_abort(void *) {}
fs3d_status fs3d_comm_init_local(fs3d_ctx *ctx, void *group, int rank)
{
    ENTRY("fs3d_comm_init_local");
    say(ctx, "fs3d_comm_init_local nranks=%d rank=%d", group ? *(int *)group : -1, rank);
    return FS3D_OK;
}

}  // extern "C"
