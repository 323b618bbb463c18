// Time statistics (FS3D_OPT_TIME_STATS, FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_TIME_STATS_EVERY, FS3D_OPT_TIME_STATS_GRAD, FS3D_OPT_TIME_STATS_WALL,
// FS3D_OPT_OUTPUT_SOURCE, FS3D_OPT_OUTPUT_MOMENT; no reference counterpart): running sums of the fields and of their products over the accumulated time steps
// of a window, and the statistic layers the result output reads in place of `next`.  The rule and its numpy twin:
// cmc_fluid_solver_amd/time_stats.py.  Per cell, nothing from a neighbour: a slab accumulates and reads out its own planes -- but for
// the gradient sums of FS3D_OPT_TIME_STATS_GRAD (k_time_grad), a stencil over `cur`, and the wall sums of FS3D_OPT_TIME_STATS_WALL
// (k_time_wall), one-sided differences at the wall cells, which whole grids alone accumulate.
// Built with -ffp-contract=off like everything outside kernels_part.hip: every operation below is rounded once in double.
#include "fs3d_common.h"

typedef float ts_f4 __attribute__((ext_vector_type(4)));
typedef double ts_d2 __attribute__((ext_vector_type(2)));
typedef unsigned ts_u4 __attribute__((ext_vector_type(4)));
typedef unsigned ts_u2 __attribute__((ext_vector_type(2)));

// the six cross sums of FS3D_OPT_TIME_STATS_CROSS: pair p is the fields (ts_pair_a(p), ts_pair_b(p)) of U, V, W, T -- uv, uw, vw, uT, vT, wT
static __device__ __forceinline__ constexpr int ts_pair_a(int p) { return p < 2 ? 0 : p == 2 ? 1 : p - 3; }
static __device__ __forceinline__ constexpr int ts_pair_b(int p) { return p == 0 ? 1 : p < 3 ? 2 : 3; }

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
// MODE 2 and 3, S2 += (double)x * (double)x; MODE 3 (FS3D_OPT_TIME_STATS_CROSS) keeps the four fields of the four cells, 16 doubles,
// and then streams the six cross sums the same way, S_ab += (double)x_a * (double)x_b for the pairs uv, uw, vw, uT, vT, wT (pair p
// at sx + p * sstride): 12 more 16-byte loads and stores, 34 against 22 per thread.  The other cells of a quad are written back as
// they were read, a quad without a NODE_IN cell is not touched.  Needs ncell % 4 == 0 and every base pointer on 16 bytes (codes: 8);
// fs3d_time_stats_accumulate decides.
// A pure stream: no LDS, no atomics, one quad per thread and no loop -- 14 (MODE 1) or 22 independent 16-byte loads in flight.
// Every access is a plain one.  The accumulators are not touched again for a whole step, so nontemporal loads and stores of them
// were the candidate: measured at 256^3 fp32 in one session they lose, 278.6 against 239.6 us in mode 1 and 503.5 against 447.1 us
// in mode 2 (profiles/time_stats_cost.txt, which says how the variant was built).
// MODE 1 and 2 are the instantiations they were: what MODE 3 adds stands under `if constexpr`, and sx is their last, unread argument.
template <typename R, int MODE>
__global__ void __launch_bounds__(256) k_time_stats_v4(const uint16_t *__restrict__ code, long long nquad, const R *__restrict__ cur,
                                                        long long fstride, unsigned *__restrict__ cnt, double *__restrict__ s1,
                                                        double *__restrict__ s2, long long sstride, double *__restrict__ sx)
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
    double xs[MODE == 3 ? 4 : 1][4];                          // MODE 3: the fields stay for the cross products
#pragma unroll
    for (int v = 0; v < 4; v++) {
        double (&x)[4] = xs[MODE == 3 ? v : 0];
        ts_load4(cur + v * fstride + l, x);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            ts_d2 *const p1 = (ts_d2 *)(s1 + v * sstride + l + 2 * h);
            ts_d2 a = *p1;
            if (in[2 * h]) a.x = a.x + x[2 * h];
            if (in[2 * h + 1]) a.y = a.y + x[2 * h + 1];
            *p1 = a;
            if constexpr (MODE >= 2) {
                ts_d2 *const p2 = (ts_d2 *)(s2 + v * sstride + l + 2 * h);
                ts_d2 b = *p2;
                if (in[2 * h]) b.x = b.x + x[2 * h] * x[2 * h];
                if (in[2 * h + 1]) b.y = b.y + x[2 * h + 1] * x[2 * h + 1];
                *p2 = b;
            }
        }
    }
    if constexpr (MODE == 3) {
#pragma unroll
        for (int p = 0; p < 6; p++) {
            const int a = ts_pair_a(p), b = ts_pair_b(p);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                ts_d2 *const px = (ts_d2 *)(sx + p * sstride + l + 2 * h);
                ts_d2 c = *px;
                if (in[2 * h]) c.x = c.x + xs[a][2 * h] * xs[b][2 * h];
                if (in[2 * h + 1]) c.y = c.y + xs[a][2 * h + 1] * xs[b][2 * h + 1];
                *px = c;
            }
        }
    }
}

// ... and cell by cell, for every cell count and alignment: the same operations on the same values
template <typename R, int MODE>
__global__ void __launch_bounds__(256) k_time_stats_v1(const uint16_t *__restrict__ code, long long ncell, const R *__restrict__ cur,
                                                        long long fstride, unsigned *__restrict__ cnt, double *__restrict__ s1,
                                                        double *__restrict__ s2, long long sstride, double *__restrict__ sx)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell || ((code[l] >> CODE_TYPE_SHIFT) & 3) != FS3D_NODE_IN) return;
    cnt[l] += 1u;
    double xs[MODE == 3 ? 4 : 1];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const double x = (double)cur[v * fstride + l];
        if constexpr (MODE == 3) xs[v] = x;
        double *const p1 = s1 + v * sstride + l;
        *p1 = *p1 + x;
        if constexpr (MODE >= 2) {
            double *const p2 = s2 + v * sstride + l;
            *p2 = *p2 + x * x;
        }
    }
    if constexpr (MODE == 3) {
#pragma unroll
        for (int p = 0; p < 6; p++) {
            double *const px = sx + p * sstride + l;
            *px = *px + xs[ts_pair_a(p)] * xs[ts_pair_b(p)];
        }
    }
}

// The statistic layer Q of one source, four fields of the context's real type, one cell per thread.  With n the steps the cell was
// NODE_IN and N the steps of the window: n >= 1 -- dn = (double)n, m_a = S1_a / dn; source 1 (mean): Q = (R)m; source 2, moment 0
// (variance): var_a = S2_a / dn - m_a * m_a, 0 where negative, Q = (R)var; source 2, moment 1 (Reynolds stresses):
// cov(a, b) = S_ab / dn - m_a * m_b, not clamped, Q_U, Q_V, Q_W = (R)cov of uv, uw, vw and Q_T = (R)(0.5 * ((var_u + var_v) + var_w));
// source 2, moment 2 (turbulent heat flux): Q_U, Q_V, Q_W = (R)cov of uT, vT, wT and Q_T = (R)var_T; source 3 (fluid fraction):
// Q_T = (R)((double)n / (double)N), Q_U = Q_V = Q_W = 0.  n = 0 -- source 1: what the cell holds in `cur` (a wall shows its node
// values as in every record); sources 2, 3: 0.  `moment` is read for source 2 only; sx only with a moment other than 0.
template <typename R>
__global__ void __launch_bounds__(256) k_time_stats_layer(int source, int moment, long long ncell, double steps, const R *__restrict__ cur,
                                                           long long fstride, const unsigned *__restrict__ cnt,
                                                           const double *__restrict__ s1, const double *__restrict__ s2,
                                                           const double *__restrict__ sx, long long sstride, R *__restrict__ q, long long qstride)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell) return;
    const unsigned n = cnt[l];
    const double dn = (double)n;
    if (source == 2 && moment != 0) {
        R r[4] = {R(0), R(0), R(0), R(0)};
        if (n) {
            double m[4], var[4];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                m[v] = s1[v * sstride + l] / dn;
                const double mm = m[v] * m[v];
                const double d = s2[v * sstride + l] / dn - mm;
                var[v] = d < 0.0 ? 0.0 : d;
            }
            double cov[6];                                    // every index below is a constant once unrolled: registers
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const double mab = m[ts_pair_a(p)] * m[ts_pair_b(p)];
                cov[p] = (p < 3) == (moment == 1) ? sx[p * sstride + l] / dn - mab : 0.0;
            }
#pragma unroll
            for (int v = 0; v < 3; v++) r[v] = (R)(moment == 1 ? cov[v] : cov[3 + v]);
            r[3] = moment == 1 ? (R)(0.5 * ((var[0] + var[1]) + var[2])) : (R)var[3];
        }
#pragma unroll
        for (int v = 0; v < 4; v++) q[v * qstride + l] = r[v];
        return;
    }
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
        q[v * qstride + l] = r;
    }
}

// FS3D_OPT_TIME_STATS_GRAD: one accumulation of the invariants of the velocity gradient (fs3d_invariants: div, Q, S:S in R) of `cur`,
// on the cells that carry them -- NODE_IN, the six neighbours inside the grid and not NODE_OUT: ng += 1, G_v += (double)value.
// Whole grids only (`cur` and `code` address the cell (0, 0, 0); no ghost plane is read).
// The form is k_div_error's: one block = the plane i = 1 .. dimx - 2 and TG_JS of the rows 1 .. dimy - 2, lanes along k in chunks of
// 256.  A thread walks down its rows with the rows j - 1, j, j + 1 of plane i in registers (three fields and the node type), takes
// the k - 1 and k + 1 values of row j from the lanes next door (the first and last lane of a wave load theirs) and loads the two
// values of the planes i - 1 and i + 1: per cell and field one new row value and two plane values, 3 loads where the plain form has
// 6, and every value of plane i comes in once per tile (plus the two rows around the tile).  The planes i +- 1 are the neighbouring
// blocks' own planes: they come through the caches.  Every address is inside the grid: i, j stay off the faces and k is clamped
// to dimz - 1 (the lanes past the line compute nothing).  The accumulators are a plain read-modify-write stream on the defined
// cells, as in k_time_stats_v4 (nontemporal accesses of them lose there).  No LDS, no atomics, no scratch.
#define TG_JS 16
template <typename R>
__global__ void __launch_bounds__(256) k_time_grad(const uint16_t *__restrict__ code, const R *__restrict__ cur, long long fstride,
                                                    int dimy, int dimz, int nj, R two_dx, R two_dy, R two_dz,
                                                    unsigned *__restrict__ cnt, double *__restrict__ gs, long long sstride)
{
    const long long plane = (long long)dimy * dimz;
    const int i = (int)(blockIdx.x / nj) + 1, j0 = (int)(blockIdx.x % nj) * TG_JS + 1;
    const int jend = j0 + TG_JS < dimy - 1 ? j0 + TG_JS : dimy - 1;
    const int lane = (int)threadIdx.x & 63;
    const R *const F[3] = {cur, cur + fstride, cur + 2 * fstride};
    auto type_at = [&](long long l) { return (int)((code[l] >> CODE_TYPE_SHIFT) & 3); };
    for (int kb = 0; kb < dimz; kb += 256) {
        const int k = kb + (int)threadIdx.x;
        const int kc = k < dimz ? k : dimz - 1;
        const bool kin = k >= 1 && k < dimz - 1;
        long long a = (long long)i * plane + (long long)(j0 - 1) * dimz + kc;
        R lo[3], mid[3], hi[3];
        int tlo = type_at(a), tmid = type_at(a + dimz);
#pragma unroll
        for (int f = 0; f < 3; f++) { lo[f] = F[f][a]; mid[f] = F[f][a + dimz]; }
        a += dimz;
        for (int j = j0; j < jend; j++, a += dimz) {          // a: the cell (i, j, kc)
            const int thi = type_at(a + dimz), txm = type_at(a - plane), txp = type_at(a + plane);
            int tkm = __shfl_up(tmid, 1, 64), tkp = __shfl_down(tmid, 1, 64);
            R xm[3], xp[3], km[3], kp[3];
#pragma unroll
            for (int f = 0; f < 3; f++) {
                hi[f] = F[f][a + dimz]; xm[f] = F[f][a - plane]; xp[f] = F[f][a + plane];
                km[f] = __shfl_up(mid[f], 1, 64); kp[f] = __shfl_down(mid[f], 1, 64);
            }
            if (lane == 0 && kc > 0) {
                tkm = type_at(a - 1);
#pragma unroll
                for (int f = 0; f < 3; f++) km[f] = F[f][a - 1];
            }
            if (lane == 63 && kc < dimz - 1) {
                tkp = type_at(a + 1);
#pragma unroll
                for (int f = 0; f < 3; f++) kp[f] = F[f][a + 1];
            }
            if (kin && tmid == FS3D_NODE_IN && tlo != FS3D_NODE_OUT && thi != FS3D_NODE_OUT && txm != FS3D_NODE_OUT &&
                txp != FS3D_NODE_OUT && tkm != FS3D_NODE_OUT && tkp != FS3D_NODE_OUT) {
                R g[3][3];
#pragma unroll
                for (int f = 0; f < 3; f++) {
                    g[f][0] = (xp[f] - xm[f]) / two_dx; g[f][1] = (hi[f] - lo[f]) / two_dy; g[f][2] = (kp[f] - km[f]) / two_dz;
                }
                R div, q, ss;
                fs3d_invariants(g, div, q, ss);
                cnt[a] += 1u;
                double *const p = gs + a;
                p[0] = p[0] + (double)div;
                p[sstride] = p[sstride] + (double)q;
                p[2 * sstride] = p[2 * sstride] + (double)ss;
            }
            tlo = tmid; tmid = thi;
#pragma unroll
            for (int f = 0; f < 3; f++) { lo[f] = mid[f]; mid[f] = hi[f]; }
        }
    }
}

// FS3D_OPT_OUTPUT_GRADIENT 2: the time means of div, Q and S:S into the fields U, V, W of a statistic layer, (R)(G / (double)ng)
// where ng >= 1 and 0 elsewhere; one cell per thread
template <typename R>
__global__ void __launch_bounds__(256) k_time_grad_layer(long long ncell, const unsigned *__restrict__ cnt, const double *__restrict__ gs,
                                                          long long sstride, R *__restrict__ q, long long qstride)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell) return;
    const unsigned n = cnt[l];
    const double dn = (double)n;
#pragma unroll
    for (int v = 0; v < 3; v++) q[v * qstride + l] = n ? (R)(gs[v * sstride + l] / dn) : R(0);
}

// FS3D_OPT_TIME_STATS_WALL: one accumulation of the wall loads (fs3d_wall_loads: tau, |tau|, q in R) of `cur` on the carriers of the
// current geometry: nw += 1, W_v += (double)value.  Whole grids only (`cur` and `code` address the cell (0, 0, 0)).
// Most cells are no walls, so this is a stream over the 2-byte code words with work on the wall cells alone: a thread takes the 8
// consecutive codes l0 .. l0 + 7 in one 16-byte load (lanes along k, a wave reads 1 KiB of the table per instruction; l0 is a
// multiple of 8 and the table is allocated on 256 bytes; the last thread of a grid whose cell count is no multiple of 8 reads its
// codes one by one) and keeps a bit per NODE_BOUND / NODE_VALVE cell.  The lanes that hold wall cells then take them one per turn,
// so a wave runs the rule as often as its busiest lane holds walls, not once per position: the cell's (x, y, z) by two divisions,
// up to three more codes and, per exposed face, the fields of the cell and of its fluid neighbour.  The sums of a cell that is no
// carrier are never read.  Plain loads and stores (the accumulators are a read-modify-write on few cells); no LDS, no atomics.
template <typename R>
__global__ void __launch_bounds__(256) k_time_wall(const uint16_t *__restrict__ code, const R *__restrict__ cur, long long fstride,
                                                    long long ncell, int dimy, int dimz, const WallRule<R> w,
                                                    unsigned *__restrict__ cnt, double *__restrict__ ws, long long sstride)
{
    const long long l0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (l0 >= ncell) return;
    unsigned mask = 0;                                         // bit q: the cell l0 + q is a wall (types 2 and 3: bit 1 of the type)
    if (l0 + 8 <= ncell) {
        const uint4 v = *reinterpret_cast<const uint4 *>(code + l0);
        const unsigned wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 8; q++) mask |= ((wd[q >> 1] >> (16 * (q & 1) + CODE_TYPE_SHIFT + 1)) & 1u) << q;
    } else
        for (int q = 0; l0 + q < ncell; q++) mask |= (((unsigned)code[l0 + q] >> (CODE_TYPE_SHIFT + 1)) & 1u) << q;
    const long long plane = (long long)dimy * dimz;
    while (mask) {
        const long long l = l0 + (__ffs((int)mask) - 1);
        mask &= mask - 1;
        const int x = (int)(l / plane);
        const long long r = l - (long long)x * plane;
        const int y = (int)(r / dimz), z = (int)(r - (long long)y * dimz);
        R tau[3], q, area;
        if (!fs3d_wall_loads(w, code, cur, cur + fstride, cur + 2 * fstride, cur + 3 * fstride, l, x, y, z, plane, dimz, (int)code[l], tau, q, area))
            continue;
        const R mag = fs3d_wall_mag(tau);
        cnt[l] += 1u;
        double *const p = ws + l;
        p[0] = p[0] + (double)tau[0];
        p[sstride] = p[sstride] + (double)tau[1];
        p[2 * sstride] = p[2 * sstride] + (double)tau[2];
        p[3 * sstride] = p[3 * sstride] + (double)mag;
        p[4 * sstride] = p[4 * sstride] + (double)q;
    }
}

// FS3D_OPT_OUTPUT_WALL 3 / 4: the time means of the wall loads into the fields U, V, W of a statistic layer, in double with
// dn = (double)nw where nw >= 1 and 0 elsewhere -- 3: (R)(W_x / dn), (R)(W_y / dn), (R)(W_z / dn); 4: (R)tawss, (R)(W_q / dn),
// (R)osi with tawss = W_mag / dn, mm the magnitude of the mean traction, osi = 0.5 * (1 - mm / tawss) where tawss > 0, else 0, and
// 0 where that is negative.  One cell per thread.
template <typename R>
__global__ void __launch_bounds__(256) k_time_wall_layer(int which, long long ncell, const unsigned *__restrict__ cnt, const double *__restrict__ ws,
                                                          long long sstride, R *__restrict__ q, long long qstride)
{
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= ncell) return;
    const unsigned n = cnt[l];
    double a = 0.0, b = 0.0, c = 0.0;
    if (n) {
        const double dn = (double)n;
        const double m[3] = {ws[l] / dn, ws[sstride + l] / dn, ws[2 * sstride + l] / dn};
        if (which == 3) { a = m[0]; b = m[1]; c = m[2]; }
        else {
            const double mm = fs3d_wall_mag(m), tawss = ws[3 * sstride + l] / dn;
            double osi = tawss > 0.0 ? 0.5 * (1.0 - mm / tawss) : 0.0;
            if (osi < 0.0) osi = 0.0;
            a = tawss; b = ws[4 * sstride + l] / dn; c = osi;
        }
    }
    q[l] = (R)a; q[qstride + l] = (R)b; q[2 * qstride + l] = (R)c;
}

static bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

template <typename R, int MODE>
static void launch_accumulate(fs3d_ctx *c)
{
    const R *const cur = (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane;      // first owned cell of field 0
    const uint16_t *const code = c->code;
    bool vec = c->ncell % 4 == 0 && aligned(code, 8) && aligned(c->ts_n.raw(), 16) && aligned(c->ts_s1.raw(), 16) &&
               (MODE < 2 || aligned(c->ts_s2.raw(), 16)) && (MODE < 3 || aligned(c->ts_sx.raw(), 16));
    for (int v = 0; v < 4; v++) vec = vec && aligned(cur + v * c->fstride, 16);
    if (vec) {
        const long long nquad = c->ncell / 4;
        hipLaunchKernelGGL((k_time_stats_v4<R, MODE>), dim3((unsigned)((nquad + 255) / 256)), dim3(256), 0, c->stream, code, nquad, cur,
                           c->fstride, (unsigned *)c->ts_n, (double *)c->ts_s1, (double *)c->ts_s2, c->ts_stride,
                           (double *)c->ts_sx);
    } else {
        hipLaunchKernelGGL((k_time_stats_v1<R, MODE>), dim3((unsigned)((c->ncell + 255) / 256)), dim3(256), 0, c->stream, code, c->ncell, cur,
                           c->fstride, (unsigned *)c->ts_n, (double *)c->ts_s1, (double *)c->ts_s2, c->ts_stride,
                           (double *)c->ts_sx);
    }
}

// FS3D_OPT_TIME_STATS_GRAD: the gradient sums of one accumulated step.  `fresh`: the step opens the window.  The two buffers are
// allocated by the first accumulation that needs them and kept; a grid without an interior cell launches nothing
static fs3d_status accumulate_gradients(fs3d_ctx *c, bool fresh)
{
    const size_t nbytes = (size_t)c->ts_stride * sizeof(unsigned), gbytes = (size_t)3 * c->ts_stride * sizeof(double);
    const bool held = c->tg_n.raw() && c->tg_g.raw();
    BUFCHK(c, c->tg_n.reserve(nbytes, &c->geom_allocs));
    BUFCHK(c, c->tg_g.reserve(gbytes, &c->geom_allocs));
    if (fresh || !held) {
        HIPCHK(c, hipMemsetAsync(c->tg_n, 0, nbytes, c->stream));
        HIPCHK(c, hipMemsetAsync(c->tg_g, 0, gbytes, c->stream));
    }
    if (c->dimx < 3 || c->dimy < 3 || c->dimz < 3) return FS3D_OK;
    const int nj = (c->dimy - 2 + TG_JS - 1) / TG_JS;
    const long long blocks = (long long)(c->dimx - 2) * nj;
    if (blocks >= (1LL << 31)) return fail(c, FS3D_ERR_UNSUPPORTED, "FS3D_OPT_TIME_STATS_GRAD: 2^31 row tiles or more");
    auto launch = [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL((k_time_grad<R>), dim3((unsigned)blocks), dim3(256), 0, c->stream, (const uint16_t *)c->code,
                           (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane, c->fstride, c->dimy, c->dimz, nj,
                           R(2) * (R)c->gdx, R(2) * (R)c->gdy, R(2) * (R)c->gdz, (unsigned *)c->tg_n, (double *)c->tg_g, c->ts_stride);
    };
    if (c->prec == FS3D_F32) launch(0.0f); else launch(0.0);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

// FS3D_OPT_TIME_STATS_WALL: the wall sums of one accumulated step, with the life of the gradient sums' buffers above
static fs3d_status accumulate_wall(fs3d_ctx *c, bool fresh)
{
    const size_t nbytes = (size_t)c->ts_stride * sizeof(unsigned), wbytes = (size_t)5 * c->ts_stride * sizeof(double);
    const bool held = c->tw_n.raw() && c->tw_w.raw();
    BUFCHK(c, c->tw_n.reserve(nbytes, &c->geom_allocs));
    BUFCHK(c, c->tw_w.reserve(wbytes, &c->geom_allocs));
    if (fresh || !held) {
        HIPCHK(c, hipMemsetAsync(c->tw_n, 0, nbytes, c->stream));
        HIPCHK(c, hipMemsetAsync(c->tw_w, 0, wbytes, c->stream));
    }
    const long long blocks = (c->ncell + 2047) / 2048;
    if (blocks >= (1LL << 31)) return fail(c, FS3D_ERR_UNSUPPORTED, "FS3D_OPT_TIME_STATS_WALL: 2^42 cells or more");
    auto launch = [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL((k_time_wall<R>), dim3((unsigned)blocks), dim3(256), 0, c->stream, (const uint16_t *)c->code,
                           (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane, c->fstride, c->ncell, c->dimy, c->dimz,
                           fs3d_wall_rule<R>(c->gdx, c->gdy, c->gdz, c->v_vis, c->t_vis), (unsigned *)c->tw_n, (double *)c->tw_w, c->ts_stride);
    };
    if (c->prec == FS3D_F32) launch(0.0f); else launch(0.0);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

fs3d_status fs3d_time_stats_accumulate(fs3d_ctx *c)
{
    // FS3D_OPT_TIME_STATS_EVERY: candidate s = 1, 2, .. of the window is taken where (s - 1) % k == 0; on the others nothing runs
    if (c->ts_candidates++ % c->opt_ts_every) return FS3D_OK;
    const bool fresh = c->ts_clear;
    const int mode = c->opt_time_stats;
    const bool cross = mode == 2 && c->opt_ts_cross;
    const size_t sbytes = (size_t)4 * c->ts_stride * sizeof(double), xbytes = (size_t)6 * c->ts_stride * sizeof(double);
    if (c->ts_clear) {
        // a new window: the buffers of the mode (kept from the window before where they exist), zeroed
        long long *const na = &c->geom_allocs;
        BUFCHK(c, c->ts_n.reserve((size_t)c->ts_stride * sizeof(unsigned), na));
        BUFCHK(c, c->ts_s1.reserve(sbytes, na));
        if (mode == 2) BUFCHK(c, c->ts_s2.reserve(sbytes, na));
        if (cross) BUFCHK(c, c->ts_sx.reserve(xbytes, na));
        HIPCHK(c, hipMemsetAsync(c->ts_n, 0, (size_t)c->ts_stride * sizeof(unsigned), c->stream));
        HIPCHK(c, hipMemsetAsync(c->ts_s1, 0, sbytes, c->stream));
        if (mode == 2) HIPCHK(c, hipMemsetAsync(c->ts_s2, 0, sbytes, c->stream));
        if (cross) HIPCHK(c, hipMemsetAsync(c->ts_sx, 0, xbytes, c->stream));
        c->ts_clear = false;
    }
    if (c->prec == FS3D_F32) { if (cross) launch_accumulate<float, 3>(c); else if (mode == 2) launch_accumulate<float, 2>(c); else launch_accumulate<float, 1>(c); }
    else { if (cross) launch_accumulate<double, 3>(c); else if (mode == 2) launch_accumulate<double, 2>(c); else launch_accumulate<double, 1>(c); }
    HIPCHK(c, hipGetLastError());
    c->ts_steps++;
    // behind the step and the sums above; a failure is the step's status, the step stands
    if (c->opt_ts_grad) { const fs3d_status st = accumulate_gradients(c, fresh); if (st != FS3D_OK) return st; }
    if (c->opt_ts_wall) return accumulate_wall(c, fresh);
    return FS3D_OK;
}

template <typename R>
static void launch_layer(fs3d_ctx *c, int source, int moment, R *q, long long qstride)
{
    const R *const cur = (const R *)c->lay[c->slot[FS3D_LAYER_CUR]] + c->plane;
    hipLaunchKernelGGL((k_time_stats_layer<R>), dim3((unsigned)((c->ncell + 255) / 256)), dim3(256), 0, c->stream, source, moment,
                       c->ncell, (double)c->ts_steps, cur, c->fstride, (const unsigned *)c->ts_n, (const double *)c->ts_s1,
                       (const double *)c->ts_s2, (const double *)c->ts_sx, c->ts_stride, q, qstride);
}

fs3d_status fs3d_time_stats_layer(fs3d_ctx *c, int source, int moment, void *q_out[4], bool *grown, bool ghost, long long *qstride_out)
{
    // `ghost`: [ghost plane][own cells][ghost plane] per field, as a layer buffer; the kernel writes the own cells either way
    const long long qstride = c->ts_stride + (ghost ? 2 * c->plane : 0), first = ghost ? c->plane : 0;
    BUFCHK(c, c->ts_q.reserve((size_t)4 * qstride * c->esize, nullptr, grown));
    char *const q = (char *)c->ts_q.raw() + (size_t)first * c->esize;
    if (c->prec == FS3D_F32) launch_layer<float>(c, source, moment, (float *)q, qstride); else launch_layer<double>(c, source, moment, (double *)q, qstride);
    HIPCHK(c, hipGetLastError());
    for (int v = 0; v < 4; v++) q_out[v] = q + (size_t)v * qstride * c->esize;
    if (qstride_out) *qstride_out = qstride;
    return FS3D_OK;
}

fs3d_status fs3d_time_stats_grad_layer(fs3d_ctx *c, void *q, long long qstride)
{
    const unsigned blocks = (unsigned)((c->ncell + 255) / 256);
    if (c->prec == FS3D_F32)
        hipLaunchKernelGGL((k_time_grad_layer<float>), dim3(blocks), dim3(256), 0, c->stream, c->ncell, (const unsigned *)c->tg_n,
                           (const double *)c->tg_g, c->ts_stride, (float *)q, qstride);
    else
        hipLaunchKernelGGL((k_time_grad_layer<double>), dim3(blocks), dim3(256), 0, c->stream, c->ncell, (const unsigned *)c->tg_n,
                           (const double *)c->tg_g, c->ts_stride, (double *)q, qstride);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

fs3d_status fs3d_time_stats_wall_layer(fs3d_ctx *c, int which, void *q, long long qstride)
{
    const unsigned blocks = (unsigned)((c->ncell + 255) / 256);
    if (c->prec == FS3D_F32)
        hipLaunchKernelGGL((k_time_wall_layer<float>), dim3(blocks), dim3(256), 0, c->stream, which, c->ncell, (const unsigned *)c->tw_n,
                           (const double *)c->tw_w, c->ts_stride, (float *)q, qstride);
    else
        hipLaunchKernelGGL((k_time_wall_layer<double>), dim3(blocks), dim3(256), 0, c->stream, which, c->ncell, (const unsigned *)c->tw_n,
                           (const double *)c->tw_w, c->ts_stride, (double *)q, qstride);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

void fs3d_time_stats_free(fs3d_ctx *c)
{
    c->ts_n.reset(&c->geom_allocs); c->ts_s1.reset(&c->geom_allocs); c->ts_s2.reset(&c->geom_allocs);
    fs3d_time_stats_free_cross(c);
    fs3d_time_stats_free_grad(c);
    fs3d_time_stats_free_wall(c);
}

void fs3d_time_stats_free_wall(fs3d_ctx *c) { c->tw_n.reset(&c->geom_allocs); c->tw_w.reset(&c->geom_allocs); }

void fs3d_time_stats_free_grad(fs3d_ctx *c) { c->tg_n.reset(&c->geom_allocs); c->tg_g.reset(&c->geom_allocs); }

void fs3d_time_stats_free_cross(fs3d_ctx *c) { c->ts_sx.reset(&c->geom_allocs); }
