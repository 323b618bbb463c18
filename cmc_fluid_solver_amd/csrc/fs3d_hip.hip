// libfs3d_hip.so -- C ABI (include/fs3d.h) of the MI355X-native FluidSolver3D hot path:
// context, geometry tables, auxiliary kernels and the time-step orchestration.
// The line-sweep kernels live in kernels_line.hip / kernels_pipe.hip, the result records in kernels_output.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "fs3d_common.h"
#include "fs3d_comm.h"

#define FS3D_VERSION "fs3d-hip 0.1 (gfx950)"

// ---------------------------------------------------------------------------------
// auxiliary kernels
// ---------------------------------------------------------------------------------

// TimeLayer3D::MergeLayerTo(grid, dest, NODE_IN) (TimeLayer3D.h:415-436, 664-683;
// GPU twin `merge`, TimeLayer3D.cu:133-146), all four fields in one pass.
template <typename R>
__global__ void __launch_bounds__(256) k_merge(const uint16_t *__restrict__ code, long long n,
                                                const R *s0, const R *s1, const R *s2, const R *s3,
                                                R *d0, R *d1, R *d2, R *d3)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (((code[i] >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN) {
            d0[i] = (d0[i] + s0[i]) / R(2);
            d1[i] = (d1[i] + s1[i]) / R(2);
            d2[i] = (d2[i] + s2[i]) / R(2);
            d3[i] = (d3[i] + s3[i]) / R(2);
        }
    }
}

// cur->CopyLayerTo(grid, next, NODE_BOUND / NODE_VALVE) (AdiSolver3D.cpp:310-311;
// TimeLayer3D.h:394-413): the BOUND/VALVE cells are a compact index list here.
template <typename R>
__global__ void __launch_bounds__(256) k_copy_list(const int *__restrict__ idx, int n,
                                                    const R *s0, const R *s1, const R *s2, const R *s3,
                                                    R *d0, R *d1, R *d2, R *d3)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { int i = idx[t]; d0[i] = s0[i]; d1[i] = s1[i]; d2[i] = s2[i]; d3[i] = s3[i]; }
}

// cur->CopyFromGrid(grid, NODE_BOUND / NODE_VALVE) (AdiSolver3D.cpp:292-293;
// TimeLayer3D.h:926-951): node values of the listed cells, stored compactly.
template <typename R>
__global__ void __launch_bounds__(256) k_impose_list(const int *__restrict__ idx, int n,
                                                      const R *v0, const R *v1, const R *v2, const R *v3,
                                                      R *d0, R *d1, R *d2, R *d3)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) { int i = idx[t]; d0[i] = v0[t]; d1[i] = v1[t]; d2[i] = v2[t]; d3[i] = v3[t]; }
}

// both of the above in one pass, for UpdateBoundaries directly followed by TimeStep (fs3d_time_step_async): the node values of the
// listed cells into cur AND next (next[i] = cur[i] = v)
template <typename R>
__global__ void __launch_bounds__(256) k_impose_list2(const int *__restrict__ idx, int n,
                                                       const R *v0, const R *v1, const R *v2, const R *v3,
                                                       R *d0, R *d1, R *d2, R *d3, R *e0, R *e1, R *e2, R *e3)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        int i = idx[t];
        const R a = v0[t], b = v1[t], c = v2[t], d = v3[t];
        d0[i] = a; d1[i] = b; d2[i] = c; d3[i] = d; e0[i] = a; e1[i] = b; e2[i] = c; e3[i] = d;
    }
}

// TimeLayer3D::EvalDivError (TimeLayer3D.h:595-641): per-cell FTYPE face sums, double
// accumulation.  Wave64 shuffle reduction, one partial (sum,count) pair per block;
// the partials are summed in a fixed order by k_div_final, so the result is
// run-to-run deterministic (it is NOT the reference's serial summation order: compare
// with a relative tolerance of ~1e-12).  A group of x-slabs gathers the partials of all global planes and sums them in
// that same order (div_error_enqueue): its error equals the single context's bit for bit where the fields do.
// (r3) One block = one plane i x DIVE_JS rows j x all k: a thread walks its k column down the rows, keeping row j-1 in
// registers and taking the k-1 values from the lane next door, so every U/V/W value is fetched once per plane pair (6 loads
// per cell instead of 24 through the caches; no integer divisions).  The per-cell expression is the reference's, term for term.
#define DIVE_JS 16
template <typename R>
__global__ void __launch_bounds__(256) k_div_error(const uint16_t *__restrict__ code,
                                                    const R *__restrict__ U, const R *__restrict__ V,
                                                    const R *__restrict__ W, int dimx, int dimy, int dimz,
                                                    int i_end, int i_skip0, R dx, R dy, R dz, double *partial, int nj)
{
    const long long plane = (long long)dimy * dimz;
    const int i = (int)(blockIdx.x / nj), j0 = (int)(blockIdx.x % nj) * DIVE_JS;
    double err = 0.0, cnt = 0.0;
    if (i < i_end && !(i_skip0 && i == 0)) {
        const R *const F[3] = {U, V, W};
        for (int kb = 0; kb < dimz; kb += 256) {
            const int k = kb + (int)threadIdx.x;
            const bool kin = k < dimz;
            const int kc = kin ? k : dimz - 1;
            // values of row j-1: [field][plane i / i-1][k / k-1]
            R pv[3][2][2];
            auto load_row = [&](int j, R (&v)[3][2][2]) __attribute__((always_inline)) {
                const long long a = (long long)i * plane + (long long)j * dimz + kc;
#pragma unroll
                for (int f = 0; f < 3; f++) {
                    const R hi = F[f][a], lo = F[f][a - plane];
                    R hm = __shfl_up(hi, 1, 64), lm = __shfl_up(lo, 1, 64);
                    if ((threadIdx.x & 63) == 0) { hm = kc > 0 ? F[f][a - 1] : hi; lm = kc > 0 ? F[f][a - plane - 1] : lo; }
                    v[f][0][0] = hi; v[f][0][1] = hm; v[f][1][0] = lo; v[f][1][1] = lm;
                }
            };
            const int jbeg = j0 > 0 ? j0 : 1;
            if (jbeg < dimy - 1 && jbeg < j0 + DIVE_JS) load_row(jbeg - 1, pv);
            for (int j = jbeg; j < j0 + DIVE_JS && j < dimy - 1; j++) {
                R cv[3][2][2];
                load_row(j, cv);
                const bool in = kin && k > 0 && k < dimz - 1 &&
                                ((code[(long long)i * plane + (long long)j * dimz + kc] >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN;
                if (in) {
                    // a = (j,k), b = (j-1,k), c = (j-1,k-1), d = (j,k-1); "- m" = plane i-1   (TimeLayer3D.h:610-632)
#define DV(f, row, pl, km) (row ? pv : cv)[f][pl][km]
                    const double ex = (double)((DV(0, 0, 0, 0) + DV(0, 1, 0, 0) + DV(0, 1, 0, 1) + DV(0, 0, 0, 1)
                                                - DV(0, 0, 1, 0) - DV(0, 1, 1, 0) - DV(0, 1, 1, 1) - DV(0, 0, 1, 1)) * dz * dy) / 4.0;
                    const double ey = (double)((DV(1, 0, 0, 0) + DV(1, 0, 1, 0) + DV(1, 0, 1, 1) + DV(1, 0, 0, 1)
                                                - DV(1, 1, 0, 0) - DV(1, 1, 1, 0) - DV(1, 1, 1, 1) - DV(1, 1, 0, 1)) * dx * dz) / 4.0;
                    const double ez = (double)((DV(2, 0, 0, 0) + DV(2, 1, 0, 0) + DV(2, 1, 1, 0) + DV(2, 0, 1, 0)
                                                - DV(2, 0, 0, 1) - DV(2, 1, 0, 1) - DV(2, 1, 1, 1) - DV(2, 0, 1, 1)) * dx * dy) / 4.0;
#undef DV
                    err += fabs(ex + ey + ez);
                    cnt += 1.0;
                }
#pragma unroll
                for (int f = 0; f < 3; f++)
#pragma unroll
                    for (int q = 0; q < 4; q++) pv[f][q >> 1][q & 1] = cv[f][q >> 1][q & 1];
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) { err += __shfl_down(err, off, 64); cnt += __shfl_down(cnt, off, 64); }
    __shared__ double se[4], sc[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { se[w] = err; sc[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (se[0] + se[1]) + (se[2] + se[3]);
        partial[2 * blockIdx.x + 1] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    }
}

// FS3D_OPT_ERR_ORDER = 1: the same per-cell terms, one per cell (0 where the reference's loop adds nothing), for the host to sum
// serially in cell order as TimeLayer3D::EvalDivError does.  Single context (no ghost planes).  Thread per cell, lanes along k.
template <typename R>
__global__ void __launch_bounds__(256) k_div_terms(const uint16_t *__restrict__ code, const R *__restrict__ U, const R *__restrict__ V,
                                                    const R *__restrict__ W, int dimx, int dimy, int dimz, R dx, R dy, R dz,
                                                    double *__restrict__ terms)
{
    const long long plane = (long long)dimy * dimz, n = plane * dimx;
    for (long long l = (long long)blockIdx.x * 256 + threadIdx.x; l < n; l += (long long)gridDim.x * 256) {
        const int i = (int)(l / plane), rem = (int)(l - (long long)i * plane), j = rem / dimz, k = rem - j * dimz;
        double t = 0.0;
        if (i >= 1 && i < dimx - 1 && j >= 1 && j < dimy - 1 && k >= 1 && k < dimz - 1 && ((code[l] >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN) {
            const long long a = l, b = l - dimz, cc = l - dimz - 1, d = l - 1;           // (j,k), (j-1,k), (j-1,k-1), (j,k-1); "- plane" = i-1
            const double ex = (double)((U[a] + U[b] + U[cc] + U[d] - U[a - plane] - U[b - plane] - U[cc - plane] - U[d - plane]) * dz * dy) / 4.0;
            const double ey = (double)((V[a] + V[a - plane] + V[d - plane] + V[d] - V[b] - V[b - plane] - V[cc - plane] - V[cc]) * dx * dz) / 4.0;
            const double ez = (double)((W[a] + W[b] + W[b - plane] + W[a - plane] - W[d] - W[cc] - W[cc - plane] - W[d - plane]) * dx * dy) / 4.0;
            t = fabs(ex + ey + ez);
        }
        terms[l] = t;
    }
}

__global__ void __launch_bounds__(256) k_div_final(const double *partial, int nblocks, double *out)
{
    __shared__ double se[256], sc[256];
    double e = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) { e += partial[2 * b]; c += partial[2 * b + 1]; }
    se[threadIdx.x] = e; sc[threadIdx.x] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { se[threadIdx.x] += se[threadIdx.x + s]; sc[threadIdx.x] += sc[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = se[0]; out[1] = sc[0]; }
}

// ---------------------------------------------------------------------------------
// context helpers
// ---------------------------------------------------------------------------------

// byte pointer to the first owned cell of field v of layer buffer buf
static char *fptr(fs3d_ctx *c, int buf, int v) { return (char *)c->lay[buf] + ((size_t)v * c->fstride + c->plane) * c->esize; }

// per-launch HIP-event timing on the context's stream (events are pooled and reused): one event pair around what a scope
// enqueues.  The end event is recorded on every way out of the scope, so rec_collect never meets a pair without one.
struct RecScope {
    fs3d_ctx *c;
    size_t end = 0;             // index of the end event; 0: no pair (timing off, or cancelled)
    RecScope(fs3d_ctx *c_, int cls) : c(c_)
    {
        if (!c->timing) return;
        if (c->ev_used + 2 > c->ev.size()) {
            hipEvent_t e0, e1;
            hipEventCreate(&e0); hipEventCreate(&e1);
            c->ev.push_back(e0); c->ev.push_back(e1);
        }
        hipEventRecord(c->ev[c->ev_used], c->stream);
        c->ev_used += 2;
        c->ev_class.push_back(cls);
        end = c->ev_used - 1;
    }
    RecScope(const RecScope &) = delete;
    ~RecScope() { if (end) hipEventRecord(c->ev[end], c->stream); }
    // nothing was launched: drop the pair (the last one begun)
    void cancel() { if (end) { c->ev_used -= 2; c->ev_class.pop_back(); end = 0; } }
};
// accumulates into t_ms/t_n (reset with fs3d_enable_timing)
void rec_collect(fs3d_ctx *c)
{
    for (size_t i = 0; i < c->ev_class.size(); i++) {
        float ms = 0;
        hipEventSynchronize(c->ev[2 * i + 1]);
        hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]);
        c->t_ms[c->ev_class[i]] += ms; c->t_n[c->ev_class[i]]++;
    }
    c->ev_used = 0; c->ev_class.clear();
}

// Device-side failures that cannot raise a HIP error (a relay hand-over of the pipe kernel that never arrived): the
// kernels set a bit in the context's pinned error word; every entry point that synchronises the stream checks it, so
// that wrong numbers are never returned with FS3D_OK (GPUplan.cpp:173-193: the reference throws on every device error).
fs3d_status check_device_errors(fs3d_ctx *c)
{
    if (!c->errw_host || *c->errw_host == 0) return FS3D_OK;
    *c->errw_host = 0;
    return fail(c, FS3D_ERR_HIP, "GPU " + std::to_string(c->device) + ": sweep kernel: a relay hand-over between waves timed out; the fields of this step are invalid");
}

// the partition kernels may be tried (results to a stated tolerance; the other kernel ids ask for one kernel or for exact bits)
static bool part_allowed(const fs3d_ctx *c) { return c->opt_kernel == FS3D_SWEEP_AUTO || c->opt_kernel == FS3D_SWEEP_PART; }

// Launch::FAILED of a sweep launcher -> FS3D_ERR_HIP with the launcher's message (c->err)
static fs3d_status launch_failed(fs3d_ctx *c, const char *what)
{
    return fail(c, FS3D_ERR_HIP, "GPU " + std::to_string(c->device) + ": " + what + ": " + c->err);
}

// ---------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------

extern "C" const char *fs3d_version(void) { return FS3D_VERSION; }

extern "C" const char *fs3d_last_error(const fs3d_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" fs3d_status fs3d_create(fs3d_ctx **out, int device, fs3d_precision prec, int dimx, int dimy, int dimz,
                                   double dx, double dy, double dz, int x_offset, int dimx_global)
{
    if (!out) return fail(nullptr, FS3D_ERR_INVALID, "fs3d_create: out is NULL");
    *out = nullptr;
    if (dimx < 1 || dimy < 3 || dimz < 3 || dimx_global < 3 || x_offset < 0 || x_offset + dimx > dimx_global)
        return fail(nullptr, FS3D_ERR_INVALID, "fs3d_create: bad dimensions");
    if (prec != FS3D_F32 && prec != FS3D_F64) return fail(nullptr, FS3D_ERR_INVALID, "fs3d_create: bad precision");
    if ((long long)(dimx + 2) * dimy * dimz >= (1LL << 31))
        return fail(nullptr, FS3D_ERR_UNSUPPORTED, "fs3d_create: slab has more than 2^31 cells");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, FS3D_ERR_HIP, "fs3d_create: no HIP device available");
    if (device < 0 || device >= ndev) return fail(nullptr, FS3D_ERR_INVALID, "fs3d_create: bad device ordinal");
    fs3d_ctx *c = new fs3d_ctx();
    c->device = device; c->prec = prec;
    c->dimx = dimx; c->dimy = dimy; c->dimz = dimz; c->x_offset = x_offset; c->dimx_global = dimx_global;
    c->gdx = dx; c->gdy = dy; c->gdz = dz;
    c->esize = prec == FS3D_F32 ? 4 : 8;
    c->plane = (long long)dimy * dimz; c->ncell = c->plane * dimx;
    c->ts_stride = (c->ncell + 3) / 4 * 4;
    if (const char *e = getenv("FS3D_TEST_DROP_HANDOFF")) c->test_drop = atoi(e) ? 1 : 0;
    if (const char *e = getenv("FS3D_DEFAULT_KERNEL")) {       // initial FS3D_OPT_SWEEP_KERNEL of new contexts (tests: 4 = bit-exact kernels only)
        const int v = atoi(e);
        if (v >= FS3D_SWEEP_AUTO && v <= FS3D_SWEEP_EXACT) c->opt_kernel = v;
    }
    if (const char *e = getenv("FS3D_DEFAULT_F64_PART")) c->opt_f64_part = atoi(e) ? 1 : 0;   // initial FS3D_OPT_F64_PART of new contexts
#define CK_FAILED(what, e) { g_create_err = call_failed(c, what, hipGetErrorString(e)); fs3d_destroy(c); return FS3D_ERR_HIP; }
#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) CK_FAILED(#call, e_) } while (0)
#define CKBUF(ok) do { if (!(ok)) CK_FAILED(#ok, hipGetLastError()) } while (0)
    CK(hipSetDevice(device));
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    // every field = haloSize + dimx*dimy*dimz + haloSize elements, data at +haloSize
    // (TimeLayer3D.h:354, GPUplan.h:79-108), zero-initialised
    // A sweep streams 16 arrays at once (4 fields of cur, temp, next, temp_out) at the same cell offset.  With power-of-two
    // grids the field stride and the allocation granularity put all 16 on the same low address bits (the same memory channel):
    // fields are padded and layers skewed against each other (FS3D_FIELD_PAD elements, FS3D_LAYER_SKEW bytes: experiments).
    // Measured (256^3 fp32, tools/pad_sweep.py, profiles/r2_padding.txt): 2338 -> 2770 Mcells/s; any pad of 576 .. 2112 elements does it.
    long long fpad = 576;                                      // 9 x 256 bytes in fp32
    size_t skew = 4864;                                        // 19 x 256 bytes per layer
    if (const char *e = getenv("FS3D_FIELD_PAD")) fpad = atoll(e) / 4 * 4;
    if (const char *e = getenv("FS3D_LAYER_SKEW")) skew = (size_t)atoll(e) / 256 * 256;
    if (fpad < 0) fpad = 0;
    c->fstride = c->ncell + 2 * c->plane + fpad;
    const size_t lbytes = (size_t)4 * c->fstride * c->esize;
    for (int l = 0; l < 5; l++) {
        CKBUF(c->lay_raw[l].replace(lbytes + 5 * skew));
        c->lay[l] = (char *)c->lay_raw[l] + (size_t)l * skew;
        CK(hipMemsetAsync(c->lay[l], 0, lbytes, c->stream));
    }
    // the 4 node-value fields and the 6 row fields of the exact kernels' scratch: padded the same way
    c->nstride = c->ncell + (getenv("FS3D_FIELD_PAD") ? fpad : 832);
    CKBUF(c->code.replace((size_t)c->nstride * sizeof(uint16_t)));
    CK(hipMemsetAsync(c->code, 0, (size_t)c->nstride * sizeof(uint16_t), c->stream));
    CKBUF(c->node.replace((size_t)4 * c->nstride * c->esize));
    CK(hipMemsetAsync(c->node, 0, (size_t)4 * c->nstride * c->esize, c->stream));
    c->red_blocks = dimx * ((dimy + DIVE_JS - 1) / DIVE_JS);      // k_div_error: one block per plane and DIVE_JS rows
    CKBUF(c->red_buf.replace(sizeof(double) * 2 * (c->red_blocks + 1)));
    CKBUF(c->red_host.replace(sizeof(double) * 2));
    CK(hipHostMalloc((void **)&c->errw_host, sizeof(int), hipHostMallocMapped));
    *c->errw_host = 0;
    CK(hipHostGetDevicePointer((void **)&c->errw_dev, c->errw_host, 0));
    CK(hipStreamSynchronize(c->stream));
#undef CKBUF
#undef CK
#undef CK_FAILED
    *out = c;
    return FS3D_OK;
}

extern "C" void fs3d_destroy(fs3d_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    fs3d_comm_destroy(c);
    fs3d_geom_destroy(c);
    if (c->errw_host) hipHostFree(c->errw_host);
    for (auto e : c->ev) hipEventDestroy(e);
    if (c->ev_src) hipEventDestroy(c->ev_src);
    if (c->ev_halo) hipEventDestroy(c->ev_halo);
    if (c->comm_stream) hipStreamDestroy(c->comm_stream);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;                                      // every buffer goes with its member (the device is still current)
}

extern "C" fs3d_status fs3d_set_params(fs3d_ctx *c, double v_T, double v_vis, double t_vis, double t_phi)
{
    if (!c) return FS3D_ERR_INVALID;
    c->v_T = v_T; c->v_vis = v_vis; c->t_vis = t_vis; c->t_phi = t_phi; c->have_params = true;
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_set_option(fs3d_ctx *c, int option, int value)
{
    if (!c) return FS3D_ERR_INVALID;
    switch (option) {
    case FS3D_OPT_SWEEP_KERNEL:
        if (value < FS3D_SWEEP_AUTO || value > FS3D_SWEEP_EXACT) return fail(c, FS3D_ERR_INVALID, "bad sweep kernel id");
        c->opt_kernel = value; return FS3D_OK;
    case FS3D_OPT_FUSE_MERGE: c->opt_fuse = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_DIV_CORE: c->opt_div_core = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_OVERLAP: c->opt_overlap = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_KEEP_TEMP: c->opt_keep_temp = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_F64_PART: c->opt_f64_part = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_ERR_ORDER: c->opt_err_order = value ? 1 : 0; return FS3D_OK;
    case FS3D_OPT_MESH_VOXELS:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad mesh voxelisation id (0: the reference's rasteriser, 1: conservative)");
        c->opt_mesh_voxels = value; return FS3D_OK;
    case FS3D_OPT_MESH_SHELL:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad mesh shell id (0: every cell whose box a triangle touches, 1: the thin shell of centre crosses)");
        c->opt_mesh_shell = value; return FS3D_OK;
    case FS3D_OPT_FRESH_CELLS:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad fresh-cells value (0: off, 1: the updates keep the node types of the geometry they replace)");
        c->opt_fresh_cells = value; return FS3D_OK;
    case FS3D_OPT_FRESH_CELLS_SLABS:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad fresh-cells-on-slabs value (0: off, 1: a slab of a group keeps the snapshot and fills with its neighbours)");
        c->opt_fresh_slabs = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_FILTER:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad output filter id (0: the reference's point sample, 1: the mean over the fluid cells of the sample's box)");
        c->opt_out_filter = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_VECTOR:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad output vector id (0: the velocity, 1: the vorticity)");
        c->opt_out_vector = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_SLABS:
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad output-on-slabs value (0: off, 1: a member of a group writes its rows of the filtered or derived record of the global grid, collectively)");
        c->opt_out_slabs = value; return FS3D_OK;
    case FS3D_OPT_TIME_STATS:
        // every call opens a new window; 0 gives the accumulators back (what the stream still does with them finishes first)
        if (value < 0 || value > 2) return fail(c, FS3D_ERR_INVALID, "bad time-statistics mode (0: off, 1: first moments, 2: first and second moments)");
        c->opt_time_stats = value; c->ts_steps = 0; c->ts_candidates = 0; c->ts_clear = true;
        if (value == 0 && c->ts_n.raw()) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            fs3d_time_stats_free(c);
        }
        return FS3D_OK;
    case FS3D_OPT_TIME_STATS_CROSS:
        // a new window as above; 0 gives the cross sums back
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad time-statistics cross value (0: off, 1: mode 2 also sums the six products uv, uw, vw, uT, vT, wT)");
        c->opt_ts_cross = value; c->ts_steps = 0; c->ts_candidates = 0; c->ts_clear = true;
        if (value == 0 && c->ts_sx.raw()) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            fs3d_time_stats_free_cross(c);
        }
        return FS3D_OK;
    case FS3D_OPT_TIME_STATS_EVERY:
        if (value < 1 || value > (1 << 20)) return fail(c, FS3D_ERR_INVALID, "bad time-statistics stride (1 .. 2^20: every k-th step of a window is accumulated, the first one always)");
        c->opt_ts_every = value; c->ts_steps = 0; c->ts_candidates = 0; c->ts_clear = true;
        return FS3D_OK;
    case FS3D_OPT_TIME_STATS_GRAD:
        // a new window as above; 0 gives the gradient sums back.  Whole grids only: the stencil would read ghost planes of `cur`,
        // which are not current after a step, and the accumulation is no collective call
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad time-statistics gradient value (0: off, 1: every accumulated step also sums div, Q and S:S of the velocity gradient)");
        if (value == 1 && (c->x_offset != 0 || c->dimx != c->dimx_global))
            return fail(c, FS3D_ERR_UNSUPPORTED, "FS3D_OPT_TIME_STATS_GRAD on an x-slab (the stencil needs the neighbours' planes of `cur` at every accumulated step)");
        c->opt_ts_grad = value; c->ts_steps = 0; c->ts_candidates = 0; c->ts_clear = true;
        if (value == 0 && (c->tg_n.raw() || c->tg_g.raw())) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            fs3d_time_stats_free_grad(c);
        }
        return FS3D_OK;
    case FS3D_OPT_TIME_STATS_WALL:
        // the contract of FS3D_OPT_TIME_STATS_GRAD: a new window; 0 gives the wall sums back; whole grids only
        if (value != 0 && value != 1) return fail(c, FS3D_ERR_INVALID, "bad time-statistics wall value (0: off, 1: every accumulated step also sums the wall shear stress and the wall heat flux)");
        if (value == 1 && (c->x_offset != 0 || c->dimx != c->dimx_global))
            return fail(c, FS3D_ERR_UNSUPPORTED, "FS3D_OPT_TIME_STATS_WALL on an x-slab (the faces across a cut need the neighbours' planes of `cur` at every accumulated step)");
        c->opt_ts_wall = value; c->ts_steps = 0; c->ts_candidates = 0; c->ts_clear = true;
        if (value == 0 && (c->tw_n.raw() || c->tw_w.raw())) {
            HIPCHK(c, hipSetDevice(c->device));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            fs3d_time_stats_free_wall(c);
        }
        return FS3D_OK;
    case FS3D_OPT_OUTPUT_WALL:
        if (value < 0 || value > 4) return fail(c, FS3D_ERR_INVALID, "bad output wall id (0: off, 1: the wall shear stress, 2: its magnitude, the wall heat flux and the area, 3 and 4: their time means)");
        c->opt_out_wall = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_GRADIENT:
        if (value < 0 || value > 2) return fail(c, FS3D_ERR_INVALID, "bad output gradient id (0: off, 1: the invariants div, Q, S:S of the sampled layer, 2: their time mean)");
        c->opt_out_gradient = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_SOURCE:
        if (value < 0 || value > 3) return fail(c, FS3D_ERR_INVALID, "bad output source id (0: `next`, 1: time mean, 2: time variance, 3: fluid fraction)");
        c->opt_out_source = value; return FS3D_OK;
    case FS3D_OPT_OUTPUT_MOMENT:
        if (value < 0 || value > 2) return fail(c, FS3D_ERR_INVALID, "bad output moment id (0: variances, 1: Reynolds stresses and k, 2: turbulent heat fluxes and var_T)");
        c->opt_out_moment = value; return FS3D_OK;
    case FS3D_OPT_XSOLVE:
        if (value < 0 || value > 3) return fail(c, FS3D_ERR_INVALID, "bad cross-slab X solve id");
        c->opt_xsolve = value; return FS3D_OK;
    default: return fail(c, FS3D_ERR_INVALID, "unknown option");
    }
}

extern "C" fs3d_status fs3d_enable_timing(fs3d_ctx *c, int on)
{
    if (!c) return FS3D_ERR_INVALID;
    c->timing = on != 0;
    c->timing_period = on > 0 ? on : 0; c->timing_steps = 0;
    for (int k = 0; k < 8; k++) { c->t_ms[k] = 0; c->t_n[k] = 0; }
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_last_step_timing(fs3d_ctx *c, float ms[4], int n[4])
{
    if (!c) return FS3D_ERR_INVALID;
    for (int k = 0; k < 3; k++) { if (ms) ms[k] = c->t_ms[k]; if (n) n[k] = c->t_n[k]; }
    float rest = 0; int nrest = 0;
    for (int k = 3; k < 8; k++) { rest += c->t_ms[k]; nrest += c->t_n[k]; }
    if (ms) ms[3] = rest;
    if (n) n[3] = nrest;
    return FS3D_OK;
}

static const char *const k_event_names[FS3D_N_EVENTS] = {"SolveSegments_Z", "SolveSegments_Y", "SolveSegments_X", "CopyLayer", "MergeLayer",
                                                         "EvalDivError", "UpdateBoundaries", "syncHalos", "CreateSegments"};
extern "C" fs3d_status fs3d_profiler_events(fs3d_ctx *c, const char *names[FS3D_N_EVENTS], float ms[FS3D_N_EVENTS], int n[FS3D_N_EVENTS])
{
    if (!c) return FS3D_ERR_INVALID;
    for (int k = 0; k < 8; k++) { if (names) names[k] = k_event_names[k]; if (ms) ms[k] = c->t_ms[k]; if (n) n[k] = c->t_n[k]; }
    if (names) names[8] = k_event_names[8];
    if (ms) ms[8] = (float)c->t_create_segments_ms;
    if (n) n[8] = c->n_create_segments;
    return FS3D_OK;
}

// ---------------------------------------------------------------------------------
// geometry: the tables of fs3d_tables.h, built on the host and written to the device
// ---------------------------------------------------------------------------------

// one table of the upload: the old buffer goes, one of the table's size comes and takes the table
static fs3d_status put_table(fs3d_ctx *c, RawBuf<DevMem> &dev, const void *src, size_t bytes)
{
    BUFCHK(c, dev.replace(bytes, &c->geom_allocs));
    HIPCHK(c, hipMemcpy(dev.raw(), src, bytes, hipMemcpyHostToDevice));
    return FS3D_OK;
}

// build (build_geom_tables: the definition of every table), refuse, put
template <typename R>
static fs3d_status upload_nodes_impl(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                     const R *vx, const R *vy, const R *vz, const R *T, int n_seg_out[3])
{
    const GeomTables t = build_geom_tables(c->dimx_global, c->dimy, c->dimz, c->x_offset, c->dimx, type, bc_vel, bc_temp);
    if (t.shared_free)
        return fail(c, FS3D_ERR_UNSUPPORTED,
                    "fs3d_upload_nodes: a cell with a FREE boundary condition closes one segment and opens the next "
                    "on the same line (two rows on one cell; the reference's result there depends on thread timing)");
    // node values of the local cells, and of the listed ones
    const R *const val[4] = {vx, vy, vz, T};
    const long long first = (long long)c->x_offset * c->plane;
    std::vector<R> bval[4];
    for (int v = 0; v < 4; v++) {
        bval[v].resize(t.bnd_idx.size());
        for (size_t q = 0; q < t.bnd_idx.size(); q++) bval[v][q] = val[v][first + t.bnd_idx[q]];
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy(c->code, t.code.data(), t.code.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->stale_in_cells = t.stale_in_cells;
    for (int d = 0; d < 3; d++) {
        GTRY(put_table(c, c->dead[d], t.dead[d].data(), t.dead[d].size()));
        if (d == 2) break;
        // exact-size tables (ucol_cap 0: fs3d_update_nodes allocates its own); none where the lines exceed UCOL_PITCH
        c->ucol[d].reset(&c->geom_allocs); c->uflag[d].reset(&c->geom_allocs);
        c->ucol_cap[d] = 0; c->n_ucol[d] = t.n_ucol[d];
        if (!t.has_columns[d]) continue;
        GTRY(put_table(c, c->ucol[d], t.ucol[d].data(), t.ucol[d].size() * sizeof(uint16_t)));
        GTRY(put_table(c, c->uflag[d], t.uflag[d].data(), t.uflag[d].size() * sizeof(unsigned)));
    }
    for (int v = 0; v < 4; v++)
        HIPCHK(c, hipMemcpy((R *)c->node + (size_t)v * c->nstride, val[v] + first, (size_t)c->ncell * sizeof(R), hipMemcpyHostToDevice));
    c->bnd_idx.reset(&c->geom_allocs);
    for (int v = 0; v < 4; v++) c->bnd_val[v].reset(&c->geom_allocs);
    c->n_bnd = (int)t.bnd_idx.size(); c->bnd_cap = c->n_bnd;
    if (c->n_bnd) {
        GTRY(put_table(c, c->bnd_idx, t.bnd_idx.data(), sizeof(int) * t.bnd_idx.size()));
        for (int v = 0; v < 4; v++) GTRY(put_table(c, c->bnd_val[v], bval[v].data(), sizeof(R) * t.bnd_idx.size()));
    }
    for (int d = 0; d < 3; d++) { c->nseg[d] = (int)t.nseg[d]; if (n_seg_out) n_seg_out[d] = (int)t.nseg[d]; }
    c->have_nodes = true; c->uploaded_once = true; c->n_create_segments++;
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_upload_nodes(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                         const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    if (!c) return FS3D_ERR_INVALID;
    if (!type || !bc_vel || !bc_temp || !vx || !vy || !vz || !T) return fail(c, FS3D_ERR_INVALID, "fs3d_upload_nodes: NULL array");
    const auto t0 = std::chrono::steady_clock::now();
    c->geom.prev_valid = false;                           // an upload is a new first geometry: no update stands behind it
    const fs3d_status st = c->prec == FS3D_F32
        ? upload_nodes_impl<float>(c, type, bc_vel, bc_temp, (const float *)vx, (const float *)vy, (const float *)vz, (const float *)T, n_seg_out)
        : upload_nodes_impl<double>(c, type, bc_vel, bc_temp, (const double *)vx, (const double *)vy, (const double *)vz, (const double *)T, n_seg_out);
    c->t_create_segments_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

// ---------------------------------------------------------------------------------
// layers
// ---------------------------------------------------------------------------------

static fs3d_status check_layer(fs3d_ctx *c, int layer)
{
    if (layer < 0 || layer > 3) return fail(c, FS3D_ERR_INVALID, "bad layer id");
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_init_layers_from_nodes(fs3d_ctx *c)
{
    if (!c) return FS3D_ERR_INVALID;
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_init_layers_from_nodes: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t lbytes = (size_t)4 * c->fstride * c->esize;
    for (int l = 0; l < 5; l++) HIPCHK(c, hipMemsetAsync(c->lay[l], 0, lbytes, c->stream));
    for (int l = 0; l < 4; l++) c->slot[l] = l;
    c->spare = 4;
    for (int v = 0; v < 4; v++)
        HIPCHK(c, hipMemcpyAsync(fptr(c, c->slot[FS3D_LAYER_CUR], v), (char *)c->node + (size_t)v * c->nstride * c->esize,
                                 (size_t)c->ncell * c->esize, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_upload_layer(fs3d_ctx *c, int layer, const void *u, const void *v, const void *w, const void *T)
{
    if (!c) return FS3D_ERR_INVALID;
    if (check_layer(c, layer)) return FS3D_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const void *src[4] = {u, v, w, T};
    for (int k = 0; k < 4; k++)
        if (src[k])
            HIPCHK(c, hipMemcpyAsync(fptr(c, c->slot[layer], k), src[k],
                                     (size_t)c->ncell * c->esize, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_download_layer(fs3d_ctx *c, int layer, void *u, void *v, void *w, void *T)
{
    if (!c) return FS3D_ERR_INVALID;
    if (check_layer(c, layer)) return FS3D_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    void *dst[4] = {u, v, w, T};
    for (int k = 0; k < 4; k++)
        if (dst[k])
            HIPCHK(c, hipMemcpyAsync(dst[k], fptr(c, c->slot[layer], k),
                                     (size_t)c->ncell * c->esize, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_field_dev_ptr(fs3d_ctx *c, int layer, int var, void **dev_ptr)
{
    if (!c || !dev_ptr) return FS3D_ERR_INVALID;
    if (check_layer(c, layer) || var < 0 || var > 3) return fail(c, FS3D_ERR_INVALID, "bad layer/var id");
    *dev_ptr = fptr(c, c->slot[layer], var);
    return FS3D_OK;
}

// ---------------------------------------------------------------------------------
// hot path
// ---------------------------------------------------------------------------------

template <typename R>
static void fill_params(fs3d_ctx *c, SweepParams<R> &p, int dir, double dt_, int b_cur, int b_temp, int b_next, int b_tout, int merge)
{
    p.dimx = c->dimx; p.dimy = c->dimy; p.dimz = c->dimz; p.plane = c->plane;
    p.cur_ = fld<R>(c, b_cur, 0); p.temp_ = fld<R>(c, b_temp, 0);
    p.next_ = fld<R>(c, b_next, 0); p.temp_out_ = fld<R>(c, b_tout, 0);
    p.fstride = c->fstride;
    p.node_ = (const R *)c->node; p.scr_ = (R *)c->scr; p.nstride = c->nstride;
    p.code = c->code;
    p.dead = c->dead[dir];
    p.ucol = dir < 2 ? c->ucol[dir] : nullptr; p.uflag = dir < 2 ? c->uflag[dir] : nullptr; p.ung = (c->dimz + 31) / 32;
    // every constant below is evaluated in FTYPE exactly as the reference writes it
    const R dx = (R)c->gdx, dy = (R)c->gdy, dz = (R)c->gdz;          // TimeLayer3D.h:1078-1080
    const R ds = dir == 0 ? dx : (dir == 1 ? dy : dz);
    const R dt = (R)dt_;                                             // FluidSolver3D.cpp:242 (FTYPE)dt
    const R v_vis = (R)c->v_vis, t_vis = (R)c->t_vis;
    p.two_ds[0] = 2 * dx; p.two_ds[1] = 2 * dy; p.two_ds[2] = 2 * dz;   // TimeLayer3D.h:338-340
    p.vis_v = v_vis / (ds * ds);                                     // AdiSolver3D.cpp:744-746
    p.vis_t = t_vis / (ds * ds);                                     // AdiSolver3D.cpp:749-751
    p.b_v = 3 / dt + 2 * p.vis_v;                                    // AdiSolver3D.cpp:761
    p.b_t = 3 / dt + 2 * p.vis_t;
    p.dt = dt; p.v_T = (R)c->v_T; p.t_phi = (R)c->t_phi;
    p.merge = merge & 3;
    p.store_next = (merge & 4) ? 0 : 1;      // merge | 4: the caller never reads this sweep's `next` (time_step_enqueue)
    p.stamps = nullptr;
    p.errw = c->errw_dev;
    p.o_begin = 0; p.o_count = 0;
    p.test_drop = c->test_drop;
    p.xiface_pass = 0;
    p.carry_in = nullptr; p.carry_out = nullptr; p.xcarry_in = nullptr; p.xcarry_out = nullptr; p.bundle0 = 0;
    p.seg_begin = 0; p.seg_len = 0; p.carry_pitch = c->plane; p.seg_index = 0; p.scr_bundles = 0;
    p.ghost_lo = c->x_offset > 0; p.ghost_hi = c->x_offset + c->dimx < c->dimx_global;
    // division core (fp32 pipe kernel): the constant divisors must be plain numbers in [2^-30, 2^60)
    // [2^-30, 2^26): with a divisor beyond 2^26 a tiny numerator gives a denormal quotient, which the core would double-round
    auto plain = [](double v) { v = v < 0 ? -v : v; return v >= 9.313225746154785e-10 && v < 67108864.0; };
    p.fast_div = c->opt_div_core && plain((double)p.two_ds[0]) && plain((double)p.two_ds[1]) && plain((double)p.two_ds[2]) && plain((double)p.dt);
}

// the rows of the thread-per-line kernels, 6 per cell: allocated by the first sweep that needs them
static fs3d_status ensure_scratch(fs3d_ctx *c) { BUFCHK(c, c->scr.reserve((size_t)6 * c->nstride * c->esize)); return FS3D_OK; }

// carry buffers of the cross-slab X sweeps ([value][line]: 6 forward, 4 backward words per line); failure is a status, not an
// early return past the callers' abort guard
static fs3d_status ensure_carries(fs3d_ctx *c)
{
    const size_t w = (size_t)c->plane * c->esize;
    if (reserve_all<DevMem>({{&c->carry[0], 6 * w}, {&c->carry[1], 6 * w}, {&c->carry[2], 4 * w}, {&c->carry[3], 4 * w}})) return FS3D_OK;
    (void)hipGetLastError();
    return fail(c, FS3D_ERR_HIP, "cross-slab X sweep: hipMalloc of the carry buffers failed");
}

// Cross-slab X sweep (nranks > 1): forward over the slabs 0 -> R-1, backward R-1 -> 0, carries over RCCL.
// The lines of the plane are cut into `xblocks` blocks that travel through the ranks as a pipeline (rank r
// works on block b while rank r+1 works on block b-1) -- the reference's `blocking` idea (AdiSolver3D.cu:642-881).
// Carries are [value][line]; a block moves as one grouped transfer of its 6 (forward) / 4 (backward) row pieces.
template <typename R>
static fs3d_status xsweep_multi(fs3d_ctx *c, SweepParams<R> &p)
{
    fs3d_status st = FS3D_OK;
    AbortOnError guard{c, &st};
    if ((st = ensure_scratch(c))) return st;
    p.scr_ = (R *)c->scr;
    const size_t pl = (size_t)c->plane;
    if ((st = ensure_carries(c))) return st;
    const bool first = c->rank == 0, last = c->rank == c->nranks - 1;
    const int nb = c->xblocks < 1 ? 1 : c->xblocks;
    // per-slab halves: the pipe kernel (rows on chip, 64 lines per bundle) where the slab allows it, else thread-per-line
    const bool pipe = c->opt_kernel != FS3D_SWEEP_LINE && xslab_pipe_supported<R>(p);
    c->ran_kernel[0] = pipe ? FS3D_SWEEP_PIPE : FS3D_SWEEP_LINE; c->ran_segmented[0] = 1;
    c->ran_xsolve = 1; c->ran_xa2a = 0;
    if (c->opt_kernel == FS3D_SWEEP_PIPE && !pipe) return fail(c, FS3D_ERR_UNSUPPORTED, "pipe kernel: slab dims unsupported for the X sweep");
    auto range = [&](int b, long long &l0, long long &l1) {
        const long long per = ((long long)pl / 64 + nb - 1) / nb * 64;      // whole waves / bundles per block
        l0 = std::min<long long>((long long)b * per, (long long)pl); l1 = std::min<long long>(l0 + per, (long long)pl);
    };
    p.carry_in = first ? nullptr : (const R *)c->carry[0]; p.carry_out = (R *)c->carry[1];
    p.xcarry_in = last ? nullptr : (const R *)c->carry[2]; p.xcarry_out = (R *)c->carry[3];
    for (int b = 0; b < nb; b++) {
        long long l0, l1; range(b, l0, l1);
        if (l1 <= l0) continue;
        if (!first && (st = fs3d_comm_xfer_rows(c, c->carry[0], 6, pl, l0, l1, c->rank - 1, false))) return st;
        if (pipe) { if (launch_xslab_pipe<R>(c, p, 1, (int)(l0 / 64), (int)(l1 / 64)) != Launch::RAN) return st = launch_failed(c, "cross-slab X sweep, forward half"); }
        else launch_xsweep_fwd<R>(c, p, first ? nullptr : c->carry[0], c->carry[1], l0, l1);
        if (!last && (st = fs3d_comm_xfer_rows(c, c->carry[1], 6, pl, l0, l1, c->rank + 1, true))) return st;
    }
    for (int b = 0; b < nb; b++) {
        long long l0, l1; range(b, l0, l1);
        if (l1 <= l0) continue;
        if (!last && (st = fs3d_comm_xfer_rows(c, c->carry[2], 4, pl, l0, l1, c->rank + 1, false))) return st;
        if (pipe) { if (launch_xslab_pipe<R>(c, p, 2, (int)(l0 / 64), (int)(l1 / 64)) != Launch::RAN) return st = launch_failed(c, "cross-slab X sweep, backward half"); }
        else launch_xsweep_bwd<R>(c, p, last ? nullptr : c->carry[2], c->carry[3], l0, l1);
        if (!first && (st = fs3d_comm_xfer_rows(c, c->carry[3], 4, pl, l0, l1, c->rank - 1, true))) return st;
    }
    return FS3D_OK;
}

// Cross-slab X sweep, reduced-interface form (kernels_line.hip: k_xiface / k_xreduce): every rank eliminates its slab at
// once, ONE all-gather of 18 words per line, then the slab's halves run with the two boundary values given -- all lines
// in one launch each, no pipeline over the ranks.
template <typename R>
static fs3d_status xsweep_reduced(fs3d_ctx *c, SweepParams<R> &p)
{
    fs3d_status st = FS3D_OK;
    AbortOnError guard{c, &st};
    if (c->nranks > FS3D_XREDUCE_MAX_RANKS) return st = fail(c, FS3D_ERR_UNSUPPORTED, "reduced-interface X solve: more than 64 slabs (k_xreduce holds the slab system in registers); use FS3D_XSOLVE_PIPELINED");
    if ((st = ensure_scratch(c))) return st;
    p.scr_ = (R *)c->scr;
    const size_t pl = (size_t)c->plane;
    if ((st = ensure_carries(c))) return st;
    const size_t xif = 18 * pl * c->esize;
    if (!stream_reserve(c, {{&c->xif_send, xif}, {&c->xif_all, c->nranks * xif}})) {
        (void)hipGetLastError();
        return st = fail(c, FS3D_ERR_HIP, "reduced-interface X solve: hipMalloc of the interface buffers failed");
    }
    // the slab's interface words: a first pass of the X partition kernel (rows and chunk elimination on chip, 8 words per cell
    // read, 18 words per line written) where it applies, else the thread-per-line walk over the planes
    bool iface_done = false;
    if (part_allowed(c)) {
        SweepParams<R> pa = p;
        pa.xiface_pass = 1; pa.carry_in = nullptr; pa.xcarry_in = nullptr; pa.carry_out = (R *)c->xif_send; pa.merge = 0; pa.store_next = 0;
        const Launch r = launch_sweep_part<R>(c, 0, pa);
        if (r == Launch::FAILED) return st = launch_failed(c, "reduced-interface X solve, interface pass");
        iface_done = r == Launch::RAN;
    }
    if (!iface_done) launch_xiface<R>(c, p, c->xif_send);
    // the R x R interface systems: every rank solves every line's (one all-gather), or -- three ranks and more -- every rank solves
    // the lines it owns and hands every rank its two boundary values (two all-to-alls of point-to-point transfers: (R-1)/R x 26
    // words per line on the wires instead of (R-1) x 18; same operations on the same values: bit-identical fields)
    const bool a2a = c->opt_xsolve == 3 || (c->opt_xsolve != 2 && c->nranks >= 3);
    c->ran_xa2a = a2a ? 1 : 0;
    if (a2a) {
        const long long lp = (((long long)pl + c->nranks - 1) / c->nranks + 63) / 64 * 64;       // lines per owner
        const size_t w1 = (size_t)c->nranks * 18 * lp * c->esize, w2 = (size_t)c->nranks * 8 * lp * c->esize;
        bool fresh = false;                        // new buffers start as zeros (the all-to-alls move the padding lines too)
        bool ok = stream_reserve(c, {{&c->xa2a[0], w1}, {&c->xa2a[1], w1}, {&c->xa2a[2], w2}, {&c->xa2a[3], w2}}, &fresh);
        for (int k = 0; k < 4 && ok && fresh; k++) ok = hipMemsetAsync(c->xa2a[k], 0, c->xa2a[k].bytes(), c->stream) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            return st = fail(c, FS3D_ERR_HIP, "distributed interface solve: hipMalloc of the exchange buffers failed");
        }
        launch_xpack<R>(c, c->xif_send, (long long)pl, lp, c->xa2a[0]);
        if ((st = fs3d_comm_alltoall(c, c->xa2a[0], c->xa2a[1], (size_t)18 * lp))) return st;
        launch_xreduce_a2a<R>(c, c->xa2a[1], (long long)pl, lp, c->nranks, c->rank, c->xa2a[2]);
        if ((st = fs3d_comm_alltoall(c, c->xa2a[2], c->xa2a[3], (size_t)8 * lp))) return st;
        launch_xunpack<R>(c, c->xa2a[3], (long long)pl, lp, c->carry[0], c->carry[2]);
    } else {
        if ((st = fs3d_comm_allgather(c, c->xif_send, c->xif_all, 18 * pl))) return st;
        launch_xreduce<R>(c, c->xif_all, (long long)pl, c->nranks, c->rank, c->carry[0], c->carry[2]);
    }
    p.carry_in = (const R *)c->carry[0]; p.carry_out = (R *)c->carry[1];
    p.xcarry_in = (const R *)c->carry[2]; p.xcarry_out = (R *)c->carry[3];
    c->ran_xsolve = iface_done ? 3 : 2;
    // the slab with both boundary values given: the X partition kernel (rows on chip, 16 words per cell) where it applies ...
    if (part_allowed(c)) {
        const Launch r = launch_sweep_part<R>(c, 0, p);
        if (r == Launch::FAILED) return st = launch_failed(c, "reduced-interface X solve, slab sweep");
        if (r == Launch::RAN) {
            c->ran_kernel[0] = FS3D_SWEEP_PART; c->ran_segmented[0] = 0;
            return FS3D_OK;
        }
    }
    // ... else the exact halves (rows through the HBM scratch)
    const bool pipe = c->opt_kernel != FS3D_SWEEP_LINE && xslab_pipe_supported<R>(p);
    c->ran_kernel[0] = pipe ? FS3D_SWEEP_PIPE : FS3D_SWEEP_LINE; c->ran_segmented[0] = 1;
    if (pipe) {
        if (launch_xslab_pipe<R>(c, p, 1, 0, (int)(pl / 64)) != Launch::RAN) return st = launch_failed(c, "reduced-interface X solve, forward half");
        if (launch_xslab_pipe<R>(c, p, 2, 0, (int)(pl / 64)) != Launch::RAN) return st = launch_failed(c, "reduced-interface X solve, backward half");
    } else {
        launch_xsweep_fwd<R>(c, p, c->carry[0], c->carry[1], 0, (long long)pl);
        launch_xsweep_bwd<R>(c, p, c->carry[2], c->carry[3], 0, (long long)pl);
    }
    return FS3D_OK;
}

// Y / Z sweep of an x-slab with the halo planes of temp travelling BESIDE the sweep (north_star: "ghost-cell halo exchange ...
// overlapped with interior-cell compute on a second HIP stream"; the reference exchanges first, TimeLayer3D.h:272-335 /
// AdiSolver3D.cpp:608).  Only the first and the last owned plane read a ghost plane (the o+-1 neighbours of the stencils):
//   stream        : interior planes [1, nx-1)  ........ wait(ev_halo) -> plane 0, plane nx-1
//   comm_stream   : wait(ev_src) -> send / recv of the 4 x 2 halo planes -> ev_halo
// ev_src marks the point where the planes to be sent are final (everything enqueued before this sweep).  Same kernels, same
// cells, same values as the plain order -- only the launches are cut differently.  false: not applicable (caller exchanges
// first and sweeps in one launch).
template <typename R>
static bool sweep_overlapped(fs3d_ctx *c, int dir, SweepParams<R> &p, int b_temp, fs3d_status &st)
{
    st = FS3D_OK;
    if (!c->opt_overlap || c->nranks < 2 || dir == 0 || c->dimx < 3) return false;
    if (!part_allowed(c) || std::is_same<R, double>::value) return false;
    if (!c->comm_stream) {
        if (hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_src, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_halo, hipEventDisableTiming) != hipSuccess) { st = fail(c, FS3D_ERR_HIP, "halo overlap: stream / event creation failed"); return true; }
    }
    if (hipEventRecord(c->ev_src, c->stream) != hipSuccess) { st = fail(c, FS3D_ERR_HIP, "halo overlap: event"); return true; }
    p.o_begin = 1; p.o_count = c->dimx - 2;
    const Launch r = launch_sweep_part<R>(c, dir, p);
    if (r == Launch::FAILED) { st = launch_failed(c, "halo overlap, interior planes"); return true; }
    if (r == Launch::NA) { p.o_begin = 0; p.o_count = 0; return false; }      // dims outside the partition kernels
    c->ran_kernel[dir] = FS3D_SWEEP_PART; c->ran_segmented[dir] = 0;
    // the interior planes are running; now the exchange, on its own stream, behind everything that was enqueued before them
    if (hipStreamWaitEvent(c->comm_stream, c->ev_src, 0) != hipSuccess) { st = fail(c, FS3D_ERR_HIP, "halo overlap: event"); return true; }
    c->xstream = c->comm_stream;
    st = fs3d_comm_halo_exchange(c, b_temp, 4);
    c->xstream = nullptr;
    if (st) return true;
    if (hipEventRecord(c->ev_halo, c->comm_stream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_halo, 0) != hipSuccess) { st = fail(c, FS3D_ERR_HIP, "halo overlap: event"); return true; }
    p.o_begin = 0; p.o_count = 1;
    launch_sweep_part<R>(c, dir, p);
    p.o_begin = c->dimx - 1; p.o_count = 1;
    launch_sweep_part<R>(c, dir, p);
    p.o_begin = 0; p.o_count = 0;
    return true;
}

// one sweep on explicit buffers; merge: 0 none, 1 fused merge, 2 fused merge twice
// halo: the temp layer's ghost planes are exchanged first -- or beside the interior planes (sweep_overlapped)
template <typename R>
static fs3d_status sweep_buffers(fs3d_ctx *c, int dir, double dt, int b_cur, int b_temp, int b_next, int b_tout, int merge, bool halo = false)
{
    SweepParams<R> p;
    fill_params<R>(c, p, dir, dt, b_cur, b_temp, b_next, b_tout, merge);
    std::fill(&c->ran_launch[dir][0][0], &c->ran_launch[dir][0][0] + 16, 0);
    const int cls = dir == 2 ? 0 : (dir == 1 ? 1 : 2);
    fs3d_status st;
    if (halo && c->nranks > 1) {
        {
            RecScope rec(c, cls);
            if (sweep_overlapped<R>(c, dir, p, b_temp, st)) {      // the exchange runs beside the interior planes: inside the sweep's time
                if (st) return st;
                HIPCHK(c, hipGetLastError());
                return FS3D_OK;
            }
            rec.cancel();
        }
        RecScope rec(c, 7);                                    // syncHalos_{X,Y,Z} (AdiSolver3D.cpp:608)
        if ((st = fs3d_comm_halo_exchange(c, b_temp, 4))) return st;
    }
    RecScope rec(c, cls);
    // (a slab context without peers that asks for the reduced form runs its kernels on the slab alone: tools/slab_cost.py times
    // what one rank computes)
    if (dir == 0 && (c->nranks > 1 || ((c->opt_xsolve == 2 || c->opt_xsolve == 3) && (p.ghost_lo || p.ghost_hi)))) {
        // reduced-interface form (all ranks at once) unless bit-equality with the sequential recurrence was asked for
        const bool reduced = c->opt_xsolve == 2 || c->opt_xsolve == 3 || (c->opt_xsolve == 0 && c->nranks <= FS3D_XREDUCE_MAX_RANKS && part_allowed(c));
        if ((st = reduced ? xsweep_reduced<R>(c, p) : xsweep_multi<R>(c, p))) return st;
        HIPCHK(c, hipGetLastError());
        return FS3D_OK;
    }
    // the first kernel that covers these dims, in the order the option allows; a launcher that failed ends the sweep
    const int ok = c->opt_kernel;
    const bool exact_fast = ok == FS3D_SWEEP_AUTO || ok == FS3D_SWEEP_EXACT || ok == FS3D_SWEEP_PIPE;
    Launch r = Launch::NA;
    int ran = FS3D_SWEEP_LINE;
    c->ran_segmented[dir] = 0;
    if (part_allowed(c)) {
        r = launch_sweep_part<R>(c, dir, p); ran = FS3D_SWEEP_PART;
        if (r == Launch::NA && ok == FS3D_SWEEP_PART) return fail(c, FS3D_ERR_UNSUPPORTED, "partition sweep kernel does not support these dims / this precision");
    }
    if (r == Launch::NA && exact_fast) { r = launch_sweep_pipe<R>(c, dir, p); ran = FS3D_SWEEP_PIPE; }
    if (r == Launch::NA && exact_fast) {
        // lines longer than one launch holds on chip: segment by segment, rows through the HBM scratch
        if ((st = ensure_scratch(c))) return st;
        p.scr_ = (R *)c->scr;
        r = launch_sweep_pipe_segmented<R>(c, dir, p);
        if (r == Launch::RAN) c->ran_segmented[dir] = 1;
    }
    if (r == Launch::NA) {
        if (ok == FS3D_SWEEP_PIPE) return fail(c, FS3D_ERR_UNSUPPORTED, "pipelined sweep kernel does not support these dims (" + c->err + ")");
        if ((st = ensure_scratch(c))) return st;
        fill_params<R>(c, p, dir, dt, b_cur, b_temp, b_next, b_tout, merge);
        launch_sweep_line<R>(c, dir, p);
        r = Launch::RAN; ran = FS3D_SWEEP_LINE;
    }
    if (r == Launch::FAILED) return launch_failed(c, "sweep");
    c->ran_kernel[dir] = ran;
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

// measurement: one pipelined sweep with per-wave phase stamps
extern "C" fs3d_status fs3d_profile_sweep(fs3d_ctx *c, int dir, double dt, int l_cur, int l_temp, int l_next,
                                          unsigned long long *stamps_out, int max_blocks, int *n_blocks_out)
{
    if (!c || !stamps_out || !n_blocks_out) return FS3D_ERR_INVALID;
    if (dir < 0 || dir > 2 || check_layer(c, l_cur) || check_layer(c, l_temp) || check_layer(c, l_next) || l_next == l_cur || l_next == l_temp)
        return fail(c, FS3D_ERR_INVALID, "fs3d_profile_sweep: bad direction or layer id");
    if (!c->have_nodes || !c->have_params) return fail(c, FS3D_ERR_INVALID, "fs3d_profile_sweep: upload nodes and set params first");
    HIPCHK(c, hipSetDevice(c->device));
    const int la = dir == 2 ? c->dimy : c->dimz, n_o = dir == 0 ? c->dimy : c->dimx;
    const int nb = n_o * ((la + 31) / 32);      // enough for the partition kernel's 32-line workgroups too
    BUFCHK(c, c->stamps.reserve(sizeof(unsigned long long) * 64 * (size_t)nb));
    HIPCHK(c, hipMemsetAsync(c->stamps, 0, sizeof(unsigned long long) * 64 * (size_t)nb, c->stream));
    Launch r = Launch::NA;
    if (c->prec == FS3D_F32) {
        SweepParams<float> p; fill_params<float>(c, p, dir, dt, c->slot[l_cur], c->slot[l_temp], c->slot[l_next], c->spare, 1);
        p.stamps = c->stamps;
        if (part_allowed(c)) r = launch_sweep_part<float>(c, dir, p);
        if (r == Launch::NA) r = launch_sweep_pipe<float>(c, dir, p);
    } else {
        SweepParams<double> p; fill_params<double>(c, p, dir, dt, c->slot[l_cur], c->slot[l_temp], c->slot[l_next], c->spare, 1);
        p.stamps = c->stamps; r = launch_sweep_pipe<double>(c, dir, p);
    }
    if (r == Launch::FAILED) return launch_failed(c, "fs3d_profile_sweep");
    if (r == Launch::NA) return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_profile_sweep: pipelined kernel does not support these dims");
    HIPCHK(c, hipGetLastError());
    const int nout = nb < max_blocks ? nb : max_blocks;
    HIPCHK(c, hipMemcpyAsync(stamps_out, c->stamps, sizeof(unsigned long long) * 64 * (size_t)nout, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_blocks_out = nout;
    return FS3D_OK;
}

template <typename R>
static fs3d_status merge_buffers(fs3d_ctx *c, int b_src, int b_dest)
{
    RecScope rec(c, 4);
    hipLaunchKernelGGL((k_merge<R>), dim3(grid_for(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell,
                       fld<R>(c, b_src, 0), fld<R>(c, b_src, 1), fld<R>(c, b_src, 2), fld<R>(c, b_src, 3),
                       fld<R>(c, b_dest, 0), fld<R>(c, b_dest, 1), fld<R>(c, b_dest, 2), fld<R>(c, b_dest, 3));
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

template <typename R>
static fs3d_status update_boundaries_impl(fs3d_ctx *c, bool also_next = false)
{
    if (!c->n_bnd) return FS3D_OK;
    const int b = c->slot[FS3D_LAYER_CUR];
    RecScope rec(c, 6);
    if (also_next) {
        const int bn = c->slot[FS3D_LAYER_NEXT];
        hipLaunchKernelGGL((k_impose_list2<R>), dim3((c->n_bnd + 255) / 256), dim3(256), 0, c->stream, c->bnd_idx, c->n_bnd,
                           (const R *)c->bnd_val[0], (const R *)c->bnd_val[1], (const R *)c->bnd_val[2], (const R *)c->bnd_val[3],
                           fld<R>(c, b, 0), fld<R>(c, b, 1), fld<R>(c, b, 2), fld<R>(c, b, 3), fld<R>(c, bn, 0), fld<R>(c, bn, 1), fld<R>(c, bn, 2), fld<R>(c, bn, 3));
    } else
    hipLaunchKernelGGL((k_impose_list<R>), dim3((c->n_bnd + 255) / 256), dim3(256), 0, c->stream, c->bnd_idx, c->n_bnd,
                       (const R *)c->bnd_val[0], (const R *)c->bnd_val[1], (const R *)c->bnd_val[2], (const R *)c->bnd_val[3],
                       fld<R>(c, b, 0), fld<R>(c, b, 1), fld<R>(c, b, 2), fld<R>(c, b, 3));
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_update_boundaries(fs3d_ctx *c)
{
    if (!c) return FS3D_ERR_INVALID;
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_update_boundaries: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    fs3d_status st = c->prec == FS3D_F32 ? update_boundaries_impl<float>(c) : update_boundaries_impl<double>(c);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

template <typename R>
static fs3d_status div_error_enqueue(fs3d_ctx *c, int layer)
{
    const int b = c->slot[layer];
    // the last slab skips its final plane (TimeLayer3D.h:606); inner slabs need the i-1 ghost (halo exchanged by caller)
    const int i_end = (c->x_offset + c->dimx == c->dimx_global) ? c->dimx - 1 : c->dimx;
    if (c->opt_err_order) {
        if (c->dimx != c->dimx_global || c->comm || c->local || c->nranks > 1)
            return fail(c, FS3D_ERR_UNSUPPORTED, "FS3D_OPT_ERR_ORDER = 1 (the CPU path's summation order) is implemented for a single context only");
        BUFCHK(c, c->err_terms.reserve((size_t)c->ncell * sizeof(double)));
    }
    // A group sums what a single context of the global grid sums, in its order: every rank writes the partial sums of its own
    // planes into their place in an array over the GLOBAL planes that is zero elsewhere, the arrays are added over the ranks
    // (div_error_finish: one non-zero term per sum, so exact), and k_div_final runs over the global array on every rank.
    const int nj = (c->dimy + DIVE_JS - 1) / DIVE_JS;
    const bool group = c->nranks > 1;
    const size_t gwords = (size_t)2 * c->dimx_global * nj;
    if (group) BUFCHK(c, c->err_parts.reserve(gwords * sizeof(double)));
    RecScope rec(c, 5);
    if (group) HIPCHK(c, hipMemsetAsync(c->err_parts, 0, gwords * sizeof(double), c->stream));
    hipLaunchKernelGGL((k_div_error<R>), dim3(c->red_blocks), dim3(256), 0, c->stream, c->code,
                       (const R *)fld<R>(c, b, 0), (const R *)fld<R>(c, b, 1), (const R *)fld<R>(c, b, 2),
                       c->dimx, c->dimy, c->dimz, i_end, c->x_offset == 0 ? 1 : 0, (R)c->gdx, (R)c->gdy, (R)c->gdz,
                       group ? c->err_parts + (size_t)2 * c->x_offset * nj : c->red_buf + 2, nj);
    if (!group) hipLaunchKernelGGL(k_div_final, dim3(1), dim3(256), 0, c->stream, c->red_buf + 2, c->red_blocks, c->red_buf);
    if (c->opt_err_order) {
        hipLaunchKernelGGL((k_div_terms<R>), dim3(grid_for(c->ncell)), dim3(256), 0, c->stream, c->code,
                           (const R *)fld<R>(c, b, 0), (const R *)fld<R>(c, b, 1), (const R *)fld<R>(c, b, 2),
                           c->dimx, c->dimy, c->dimz, (R)c->gdx, (R)c->gdy, (R)c->gdz, c->err_terms);
    }
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

static fs3d_status div_error_finish(fs3d_ctx *c, double *err, long long *count)
{
    if (c->nranks > 1) {                                        // the partial sums of all global planes, then the single context's final sum
        const int gblocks = c->dimx_global * ((c->dimy + DIVE_JS - 1) / DIVE_JS);
        fs3d_status st = fs3d_comm_allreduce_sum(c, c->err_parts, (size_t)2 * gblocks);
        if (st) return st;
        hipLaunchKernelGGL(k_div_final, dim3(1), dim3(256), 0, c->stream, c->err_parts, gblocks, c->red_buf);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(c->red_host, c->red_buf, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (c->opt_err_order) {
        // TimeLayer3D.h:604-628: err += fabs(...) cell after cell; adding the 0.0 of a cell the loop skips changes nothing
        c->err_terms_host.resize((size_t)c->ncell);
        HIPCHK(c, hipMemcpyAsync(c->err_terms_host.data(), c->err_terms, (size_t)c->ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        double sum = 0.0;
        for (double t : c->err_terms_host) sum += t;
        c->red_host[0] = sum;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (count) *count = (long long)c->red_host[1];
    if (err) *err = c->red_host[0] / c->red_host[1];   // err / count (0/0 = NaN as in the reference)
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_eval_div_error(fs3d_ctx *c, int layer, double *err_out, long long *count_out)
{
    if (!c) return FS3D_ERR_INVALID;
    if (check_layer(c, layer)) return FS3D_ERR_INVALID;
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_eval_div_error: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    fs3d_status st = fs3d_comm_halo_exchange(c, c->slot[layer], 3);   // U,V,W ghosts (TimeLayer3D.h:601-603)
    if (st) return st;
    st = c->prec == FS3D_F32 ? div_error_enqueue<float>(c, layer) : div_error_enqueue<double>(c, layer);
    if (st) return st;
    return div_error_finish(c, err_out, count_out);
}

extern "C" fs3d_status fs3d_sweep(fs3d_ctx *c, int dir, double dt, int l_cur, int l_temp, int l_next, int merge_into_temp)
{
    if (!c) return FS3D_ERR_INVALID;
    if (dir < 0 || dir > 2 || check_layer(c, l_cur) || check_layer(c, l_temp) || check_layer(c, l_next))
        return fail(c, FS3D_ERR_INVALID, "fs3d_sweep: bad direction or layer id");
    if (!c->have_nodes || !c->have_params) return fail(c, FS3D_ERR_INVALID, "fs3d_sweep: upload nodes and set params first");
    if (l_next == l_cur || l_next == l_temp) return fail(c, FS3D_ERR_INVALID, "fs3d_sweep: next must differ from cur and temp");
    HIPCHK(c, hipSetDevice(c->device));
    fs3d_status st = fs3d_comm_halo_exchange(c, c->slot[l_temp], 4);   // temp->syncHalos (AdiSolver3D.cpp:608)
    if (st) return st;
    const bool f32 = c->prec == FS3D_F32;
    if (merge_into_temp && c->opt_fuse) {
        const int bt = c->slot[l_temp], bo = c->spare;
        st = f32 ? sweep_buffers<float>(c, dir, dt, c->slot[l_cur], bt, c->slot[l_next], bo, 1)
                 : sweep_buffers<double>(c, dir, dt, c->slot[l_cur], bt, c->slot[l_next], bo, 1);
        if (st) return st;
        c->slot[l_temp] = bo; c->spare = bt;
    } else {
        const int bt = c->slot[l_temp];
        st = f32 ? sweep_buffers<float>(c, dir, dt, c->slot[l_cur], bt, c->slot[l_next], bt, 0)
                 : sweep_buffers<double>(c, dir, dt, c->slot[l_cur], bt, c->slot[l_next], bt, 0);
        if (st) return st;
        if (merge_into_temp) {
            st = f32 ? merge_buffers<float>(c, c->slot[l_next], bt) : merge_buffers<double>(c, c->slot[l_next], bt);
            if (st) return st;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ev_used) rec_collect(c);
    return check_device_errors(c);
}

extern "C" fs3d_status fs3d_merge(fs3d_ctx *c, int l_src, int l_dest)
{
    if (!c) return FS3D_ERR_INVALID;
    if (check_layer(c, l_src) || check_layer(c, l_dest) || l_src == l_dest) return fail(c, FS3D_ERR_INVALID, "fs3d_merge: bad layers");
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_merge: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    fs3d_status st = c->prec == FS3D_F32 ? merge_buffers<float>(c, c->slot[l_src], c->slot[l_dest])
                                         : merge_buffers<double>(c, c->slot[l_src], c->slot[l_dest]);
    if (st) return st;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

// AdiSolver3D::TimeStep, AdiSolver3D.cpp:306-391, enqueued on the context's stream.
template <typename R>
static fs3d_status time_step_enqueue(fs3d_ctx *c, double dt, int G, int L, bool compute_error, bool bnd_copied = false)
{
    const int bCur = c->slot[FS3D_LAYER_CUR], bNext = c->slot[FS3D_LAYER_NEXT], bHalf = c->slot[FS3D_LAYER_HALF];
    fs3d_status st;
    // :310-311  cur -> next on NODE_BOUND and NODE_VALVE
    if (c->n_bnd && !bnd_copied) {
        RecScope rec(c, 3);
        hipLaunchKernelGGL((k_copy_list<R>), dim3((c->n_bnd + 255) / 256), dim3(256), 0, c->stream, c->bnd_idx, c->n_bnd,
                           (const R *)fld<R>(c, bCur, 0), (const R *)fld<R>(c, bCur, 1), (const R *)fld<R>(c, bCur, 2), (const R *)fld<R>(c, bCur, 3),
                           fld<R>(c, bNext, 0), fld<R>(c, bNext, 1), fld<R>(c, bNext, 2), fld<R>(c, bNext, 3));
    }
    const bool fuse = c->opt_fuse && L >= 1 && G >= 1;
    if (!fuse) {
        // :320 cur->CopyLayerTo(temp)
        {
            RecScope rec(c, 3);
            for (int v = 0; v < 4; v++)
                HIPCHK(c, hipMemcpyAsync(fld<R>(c, c->slot[FS3D_LAYER_TEMP], v), fld<R>(c, bCur, v), (size_t)c->ncell * sizeof(R),
                                         hipMemcpyDeviceToDevice, c->stream));
        }
        for (int it = 0; it < G; it++) {
            const int bT = c->slot[FS3D_LAYER_TEMP];
            const int plan[3][3] = {{2, bCur, bNext}, {1, bNext, bHalf}, {0, bHalf, bNext}};   // :338, :342, :343
            for (int d = 0; d < 3; d++)
                for (int l = 0; l < L; l++) {
                    if ((st = fs3d_comm_halo_exchange(c, bT, 4))) return st;
                    if ((st = sweep_buffers<R>(c, plan[d][0], dt, plan[d][1], bT, plan[d][2], bT, 0))) return st;
                    if ((st = merge_buffers<R>(c, plan[d][2], bT))) return st;                 // :651
                }
            if ((st = merge_buffers<R>(c, bNext, bT))) return st;                               // :354
        }
    } else {
        // Fused form.  The sweep kernel writes next and the merged temp in one pass
        // (temp is double-buffered so cross-line stencil reads still see the un-merged temp);
        // the first sweep reads temp straight from cur (saves the :320 copy); the last X
        // sweep of each global iteration applies the :354 merge as a second averaging step.
        int bTin = bCur;                       // temp == cur until the first merge
        int bTout = c->slot[FS3D_LAYER_TEMP];
        int bSpare = c->spare;
        for (int it = 0; it < G; it++) {
            const int plan[3][3] = {{2, bCur, bNext}, {1, bNext, bHalf}, {0, bHalf, bNext}};
            for (int d = 0; d < 3; d++)
                for (int l = 0; l < L; l++) {
                    // `next` of a local iteration that is not the last of its direction is overwritten by the following
                    // one without having been read (the merge into temp is fused into the kernel): not stored
                    // (r3) ... and so is the `next` of the X sweep that closes a global iteration but the last: the Z sweep of the
                    // following iteration writes `next` on every segment cell before anything reads it (Y reads it as its `cur` on
                    // interior rows only; the result layer is the LAST iteration's) -- provided no NODE_IN cell relies on stale values
                    const bool x_dead = d == 2 && l == L - 1 && it < G - 1 && c->stale_in_cells == 0;
                    int merge = ((d == 2 && l == L - 1) ? 2 : 1) | ((l < L - 1 || x_dead) ? 4 : 0);
                    // (r3) the merged temp of the step's very last sweep is dead too: the next step starts from temp := cur (:320),
                    // GetLayer / EvalDivError read `next` (FS3D_OPT_KEEP_TEMP 1 stores it, as the reference's private member holds it)
                    const bool last_sweep = it == G - 1 && d == 2 && l == L - 1;
                    if (last_sweep && !c->opt_keep_temp && bTin != bCur) merge = 0;
                    if ((st = sweep_buffers<R>(c, plan[d][0], dt, plan[d][1], bTin, plan[d][2], merge ? bTout : bTin, merge, true))) return st;
                    if (merge == 0) continue;                                  // temp stays where it is
                    if (bTin == bCur) { bTin = bTout; bTout = bSpare; }
                    else { int t = bTin; bTin = bTout; bTout = t; }
                }
        }
        c->slot[FS3D_LAYER_TEMP] = bTin; c->spare = bTout;
    }
    if (compute_error) {
        if ((st = fs3d_comm_halo_exchange(c, bNext, 3))) return st;
        if ((st = div_error_enqueue<R>(c, FS3D_LAYER_NEXT))) return st;
    }
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_time_step(fs3d_ctx *c, double dt, int G, int L, int compute_error, double *err_out)
{
    if (!c) return FS3D_ERR_INVALID;
    if (!c->have_nodes || !c->have_params) return fail(c, FS3D_ERR_INVALID, "fs3d_time_step: upload nodes and set params first");
    if (G < 0 || L < 0 || !(dt > 0)) return fail(c, FS3D_ERR_INVALID, "fs3d_time_step: bad dt / iteration counts");
    if (c->opt_ts_grad && c->opt_time_stats && c->nranks > 1)
        return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_time_step: FS3D_OPT_TIME_STATS_GRAD on a member of a group (the gradient sums are not collective)");
    if (c->opt_ts_wall && c->opt_time_stats && c->nranks > 1)
        return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_time_step: FS3D_OPT_TIME_STATS_WALL on a member of a group (the wall sums are not collective)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->timing_period > 1) c->timing = (c->timing_steps++ % c->timing_period) == 0;      // sampled timing: every N-th time step carries the events
    fs3d_status st = c->prec == FS3D_F32 ? time_step_enqueue<float>(c, dt, G, L, compute_error != 0)
                                         : time_step_enqueue<double>(c, dt, G, L, compute_error != 0);
    if (st) return st;
    if (compute_error) {
        double e = 0;
        if ((st = div_error_finish(c, &e, nullptr))) return st;
        c->diffError = e;                                                    // :366
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (c->ev_used) rec_collect(c);
    if ((st = check_device_errors(c))) return st;
    if (err_out) *err_out = c->diffError;
    if (c->diffError > 0.01) {                                               // :371-374 (ERR_THRESHOLD, AdiSolver3D.h:32)
        char b[128]; snprintf(b, sizeof b, "Error is too big! %f", c->diffError);
        return fail(c, FS3D_ERR_DIVERGED, b);
    }
    std::swap(c->slot[FS3D_LAYER_CUR], c->slot[FS3D_LAYER_NEXT]);            // :388-390
    if (c->opt_time_stats) return fs3d_time_stats_accumulate(c);             // the new `cur` joins the window (enqueued)
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_time_step_async(fs3d_ctx *c, double dt, int G, int L)
{
    if (!c) return FS3D_ERR_INVALID;
    if (!c->have_nodes || !c->have_params) return fail(c, FS3D_ERR_INVALID, "fs3d_time_step_async: upload nodes and set params first");
    if (G < 0 || L < 0 || !(dt > 0)) return fail(c, FS3D_ERR_INVALID, "fs3d_time_step_async: bad dt / iteration counts");
    if (c->opt_ts_grad && c->opt_time_stats && c->nranks > 1)
        return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_time_step_async: FS3D_OPT_TIME_STATS_GRAD on a member of a group (the gradient sums are not collective)");
    if (c->opt_ts_wall && c->opt_time_stats && c->nranks > 1)
        return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_time_step_async: FS3D_OPT_TIME_STATS_WALL on a member of a group (the wall sums are not collective)");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->timing_period > 1) c->timing = (c->timing_steps++ % c->timing_period) == 0;
    // UpdateBoundaries and the cur -> next copy of the boundary cells that opens TimeStep: one pass over the list
    fs3d_status st = c->prec == FS3D_F32 ? update_boundaries_impl<float>(c, true) : update_boundaries_impl<double>(c, true);
    if (st) return st;
    st = c->prec == FS3D_F32 ? time_step_enqueue<float>(c, dt, G, L, false, true) : time_step_enqueue<double>(c, dt, G, L, false, true);
    if (st) return st;
    std::swap(c->slot[FS3D_LAYER_CUR], c->slot[FS3D_LAYER_NEXT]);
    if (c->opt_time_stats) return fs3d_time_stats_accumulate(c);
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_last_sweep_kernel(fs3d_ctx *c, int dir, int *kernel_out, int *segmented_out)
{
    if (!c || dir < 0 || dir > 2 || !kernel_out) return FS3D_ERR_INVALID;
    *kernel_out = c->ran_kernel[dir];
    if (segmented_out) *segmented_out = c->ran_segmented[dir] | (dir == 0 ? (c->ran_xsolve << 1) | (c->ran_xa2a << 3) : 0);
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_last_sweep_launch(fs3d_ctx *c, int dir, int pass, int out[8])
{
    if (!c || dir < 0 || dir > 2 || pass < 0 || pass > 1 || !out) return FS3D_ERR_INVALID;
    std::copy(c->ran_launch[dir][pass], c->ran_launch[dir][pass] + 8, out);
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_synchronize(fs3d_ctx *c)
{
    if (!c) return FS3D_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ev_used) rec_collect(c);
    return check_device_errors(c);
}
