// Time statistics (FS3D_OPT_TIME_STATS, FS3D_OPT_OUTPUT_SOURCE; no reference counterpart): running sums of the fields over the
// time steps of a window, and the statistic layers the result output reads in place of `next`.  The rule and its numpy twin:
// cmc_fluid_solver_amd/time_stats.py.  Per cell, nothing from a neighbour: a slab accumulates and reads out its own planes.
// Built with -ffp-contract=off like everything outside kernels_part.hip: every operation below is rounded once in double.
#include "fs3d_common.h"

typedef float ts_f4 __attribute__((ext_vector_type(4)));
typedef double ts_d2 __attribute__((ext_vector_type(2)));
typedef unsigned ts_u4 __attribute__((ext_vector_type(4)));
typedef unsigned ts_u2 __attribute__((ext_vector_type(2)));

// four consecutive values of a field, widened to double
static __device__ __forceinline__ void ts_load4(const float *p, double (&x)[4])
{
    const ts_f4 v = *(const ts_f4 *)p;
    x[0] = (double)v.x; x[1] = (double)v.y; x[2] = (double)v.z; x[3] = (double)v.w;
}
static __device__ __forceinline__ void ts_load4(const double *p, double (&x)[4])
{
    const ts_d2 a = *(const ts_d2 *)p, b = *(const ts_d2 *)(p + 2);
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
}

// One accumulation, vector form: a thread owns the four consecutive cells [4q, 4q + 4) -- 8 bytes of codes, 16 bytes of counts, per
// field 16 (fp32) or 2 x 16 (fp64) bytes of `cur` and 2 x 16 bytes of every sum.  On the NODE_IN cells n += 1, S1 += (double)x and,
// MODE 2, S2 += (double)x * (double)x; the other cells of a quad are written back as they were read, a quad without a NODE_IN cell
// is not touched.  Needs ncell % 4 == 0 and every base pointer on 16 bytes (codes: 8); fs3d_time_stats_accumulate decides.
// A pure stream: no LDS, no atomics, one quad per thread and no loop -- 14 (MODE 1) or 22 independent 16-byte loads in flight.
// Every access is a plain one.  The accumulators are not touched again for a whole step, so nontemporal loads and stores of them
// were the candidate: measured at 256^3 fp32 in one session they lose, 278.6 against 239.6 us in mode 1 and 503.5 against 447.1 us
// in mode 2 (profiles/time_stats_cost.txt, which says how the variant was built).
template <typename R, int MODE>
__global__ void __launch_bounds__(256) k_time_stats_v4(const uint16_t *__restrict__ code, long long nquad, const R *__restrict__ cur,
                                                        long long fstride, unsigned *__restrict__ cnt, double *__restrict__ s1,
                                                        double *__restrict__ s2, long long sstride)
{
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nquad) return;
    const long long l = 4 * q;
    const ts_u2 cw = *(const ts_u2 *)(code + l);
    const bool in[4] = {((cw.x >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN, ((cw.x >> (16 + CODE_TYPE_SHIFT)) & 3) == FS3D_NODE_IN,
                        ((cw.y >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN, ((cw.y >> (16 + CODE_TYPE_SHIFT)) & 3) == FS3D_NODE_IN};
    if (!(in[0] || in[1] || in[2] || in[3])) return;
    ts_u4 n = *(const ts_u4 *)(cnt + l);
    n.x += in[0]; n.y += in[1]; n.z += in[2]; n.w += in[3];
    *(ts_u4 *)(cnt + l) = n;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        double x[4];
        ts_load4(cur + v * fstride + l, x);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            ts_d2 *const p1 = (ts_d2 *)(s1 + v * sstride + l + 2 * h);
            ts_d2 a = *p1;
            if (in[2 * h]) a.x = a.x + x[2 * h];
            if (in[2 * h + 1]) a.y = a.y + x[2 * h + 1];
            *p1 = a;
            if constexpr (MODE == 2) {
                ts_d2 *const p2 = (ts_d2 *)(s2 + v * sstride + l + 2 * h);
                ts_d2 b = *p2;
                if (in[2 * h]) b.x = b.x + x[2 * h] * x[2 * h];
                if (in[2 * h + 1]) b.y = b.y + x[2 * h + 1] * x[2 * h + 1];
                *p2 = b;
            }
        }
    }
}

// ... and cell by cell, for every cell count and alignment: the same operations on the same values
template <typename R, int MODE>
__global__ void __launch_bounds__(256) k_time_stats_v1(const uint16_t *__restrict__ code, long long ncell, const R *__restrict__ cur,
                                                        long long fstride, unsigned *__restrict__ cnt, double *__restrict__ s1,
                                                        double *__restrict__ s2, long long sstride)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell || ((code[l] >> CODE_TYPE_SHIFT) & 3) != FS3D_NODE_IN) return;
    cnt[l] += 1u;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const double x = (double)cur[v * fstride + l];
        double *const p1 = s1 + v * sstride + l;
        *p1 = *p1 + x;
        if constexpr (MODE == 2) {
            double *const p2 = s2 + v * sstride + l;
            *p2 = *p2 + x * x;
        }
    }
}

// The statistic layer Q of one source, four fields of the context's real type, one cell per thread.  With n the steps the cell was
// NODE_IN and N the steps of the window: n >= 1 -- m = S1 / (double)n; source 1 (mean): Q = (R)m; source 2 (variance):
// v = S2 / (double)n - m * m, 0 where negative, Q = (R)v; source 3 (fluid fraction): Q_T = (R)((double)n / (double)N), Q_U = Q_V =
// Q_W = 0.  n = 0 -- source 1: what the cell holds in `cur` (a wall shows its node values as in every record); sources 2, 3: 0.
template <typename R>
__global__ void __launch_bounds__(256) k_time_stats_layer(int source, long long ncell, double steps, const R *__restrict__ cur,
                                                           long long fstride, const unsigned *__restrict__ cnt,
                                                           const double *__restrict__ s1, const double *__restrict__ s2,
                                                           long long sstride, R *__restrict__ q)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell) return;
    const unsigned n = cnt[l];
    const double dn = (double)n;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        R r = R(0);
        if (source == 1) {
            r = n ? (R)(s1[v * sstride + l] / dn) : cur[v * fstride + l];
        } else if (source == 2) {
            if (n) {
                const double m = s1[v * sstride + l] / dn;
                const double mm = m * m;
                const double var = s2[v * sstride + l] / dn - mm;
                r = (R)(var < 0.0 ? 0.0 : var);
            }
        } else if (v == 3 && n) {
            r = (R)(dn / steps);
        }
        q[v * sstride + l] = r;
    }
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename R, int MODE>
static void launch_accumulate(fs3d_ctx *c)
{
    const R *const cur = (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane;      // first owned cell of field 0
    const uint16_t *const code = c->code;
    bool vec = c->ncell % 4 == 0 && aligned(code, 8) && aligned(c->ts_n.raw(), 16) && aligned(c->ts_s1.raw(), 16) &&
               (MODE < 2 || aligned(c->ts_s2.raw(), 16));
    for (int v = 0; v < 4; v++) vec = vec && aligned(cur + v * c->fstride, 16);
    if (vec) {
        const long long nquad = c->ncell / 4;
        hipLaunchKernelGGL((k_time_stats_v4<R, MODE>), dim3((unsigned)((nquad + 255) / 256)), dim3(256), 0, c->stream, code, nquad, cur,
                           c->fstride, (unsigned *)c->ts_n, (double *)c->ts_s1, (double *)c->ts_s2, c->ts_stride);
    } else {
        hipLaunchKernelGGL((k_time_stats_v1<R, MODE>), dim3((unsigned)((c->ncell + 255) / 256)), dim3(256), 0, c->stream, code, c->ncell, cur,
                           c->fstride, (unsigned *)c->ts_n, (double *)c->ts_s1, (double *)c->ts_s2, c->ts_stride);
    }
}

fs3d_status fs3d_time_stats_accumulate(fs3d_ctx *c)
{
    const int mode = c->opt_time_stats;
    const size_t sbytes = (size_t)4 * c->ts_stride * sizeof(double);
    if (c->ts_clear) {
        // a new window: the buffers of the mode (kept from the window before where they exist), zeroed
        long long *const na = &c->geom_allocs;
        BUFCHK(c, c->ts_n.reserve((size_t)c->ts_stride * sizeof(unsigned), na));
        BUFCHK(c, c->ts_s1.reserve(sbytes, na));
        if (mode == 2) BUFCHK(c, c->ts_s2.reserve(sbytes, na));
        HIPCHK(c, hipMemsetAsync(c->ts_n, 0, (size_t)c->ts_stride * sizeof(unsigned), c->stream));
        HIPCHK(c, hipMemsetAsync(c->ts_s1, 0, sbytes, c->stream));
        if (mode == 2) HIPCHK(c, hipMemsetAsync(c->ts_s2, 0, sbytes, c->stream));
        c->ts_clear = false;
    }
    if (c->prec == FS3D_F32) { if (mode == 2) launch_accumulate<float, 2>(c); else launch_accumulate<float, 1>(c); }
    else { if (mode == 2) launch_accumulate<double, 2>(c); else launch_accumulate<double, 1>(c); }
    HIPCHK(c, hipGetLastError());
    c->ts_steps++;
    return FS3D_OK;
}

template <typename R>
static void launch_layer(fs3d_ctx *c, int source)
{
    const R *const cur = (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane;
    hipLaunchKernelGGL((k_time_stats_layer<R>), dim3((unsigned)((c->ncell + 255) / 256)), dim3(256), 0, c->stream, source, c->ncell,
                       (double)c->ts_steps, cur, c->fstride, (const unsigned *)c->ts_n, (const double *)c->ts_s1, (const double *)c->ts_s2,
                       c->ts_stride, (R *)c->ts_q);
}

fs3d_status fs3d_time_stats_layer(fs3d_ctx *c, int source, void *q_out[4], bool *grown)
{
    BUFCHK(c, c->ts_q.reserve((size_t)4 * c->ts_stride * c->esize, nullptr, grown));
    if (c->prec == FS3D_F32) launch_layer<float>(c, source); else launch_layer<double>(c, source);
    HIPCHK(c, hipGetLastError());
    for (int v = 0; v < 4; v++) q_out[v] = (char *)c->ts_q.raw() + (size_t)v * c->ts_stride * c->esize;
    return FS3D_OK;
}

void fs3d_time_stats_free(fs3d_ctx *c)
{
    c->ts_n.reset(&c->geom_allocs); c->ts_s1.reset(&c->geom_allocs); c->ts_s2.reset(&c->geom_allocs);
}
