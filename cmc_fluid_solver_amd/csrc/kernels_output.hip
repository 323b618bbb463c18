// Result records (fs3d_get_layer, _rows, _dev, _info of include/fs3d.h): the stamp, the gather behind GetLayer, the box-mean filter,
// the vorticity, the invariants of the velocity gradient and (whole grids only) the wall loads, on a whole grid and -- as one collective call, FS3D_OPT_OUTPUT_SLABS -- on the x-slabs of a group.  One kernel per
// stage and one host body: a whole grid is the slab x_offset = 0, dimx = dimx_global of a group of one, with no straddling row.
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "fs3d_common.h"
#include "fs3d_comm.h"

// TimeLayer3D::Clear(grid, NODE_OUT, MISSING_VALUE x4) (TimeLayer3D.h:974-999; `clear`, TimeLayer3D.cu:98-116)
template <typename R>
__global__ void __launch_bounds__(256) k_clear_type(const uint16_t *__restrict__ code, long long n, int type, R val,
                                                     R *d0, R *d1, R *d2, R *d3)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        if (((code[i] >> CODE_TYPE_SHIFT) & 3) == type) { d0[i] = val; d1[i] = val; d2[i] = val; d3[i] = val; }
}

// TimeLayer3D::FilterToArrays (TimeLayer3D.h:819-924): the nearest-neighbour samples of one layer, out[i,j,k] = layer[i*gx/odx,
// j*dimy/ody, k*dimz/odz], into outV (interleaved x, y, z) and outT (double).  A pure gather: order-free, bit-exact.  One thread
// per sample, k fastest: blockIdx.x = output row i - i0, the threads of a row walk its ody*odz samples (a wave stores 64 x 3
// consecutive R and 64 consecutive doubles).  The slab holds the planes [x_offset, x_offset + dimx) of gx and writes the rows
// [i0, i1) whose source plane it owns; outV / outT address the first sample of row i0.  Runs behind k_clear_type on the same
// stream and reads the stamped values.
template <typename R>
__global__ void __launch_bounds__(256) k_get_layer(const R *__restrict__ U, const R *__restrict__ V, const R *__restrict__ W,
                                                    const R *__restrict__ T, int x_offset, int dimx, long long plane, int dimy, int dimz,
                                                    int gx, int odx, int ody, int odz, int i0, int i1,
                                                    R *__restrict__ outV, double *__restrict__ outT)
{
    const int i = i0 + (int)blockIdx.x;
    const int x = (int)((long long)i * gx / odx) - x_offset;
    if (i >= i1 || x < 0 || x >= dimx) return;
    const unsigned po = (unsigned)ody * (unsigned)odz;
    for (unsigned p = blockIdx.y * 256u + threadIdx.x; p < po; p += gridDim.y * 256u) {
        const unsigned j = p / (unsigned)odz, k = p - j * (unsigned)odz;
        const int y = (int)((long long)j * dimy / ody), z = (int)((long long)k * dimz / odz);
        const long long id = (long long)x * plane + (long long)y * dimz + z;
        const long long ind = (long long)blockIdx.x * po + p;
        outV[3 * ind] = U[id]; outV[3 * ind + 1] = V[id]; outV[3 * ind + 2] = W[id];
        outT[ind] = (double)T[id];
    }
}

// What a slab knows of the grid, for the box kernel and the finishing one: its planes [x_offset, x_offset + dimx) of gx, the fields
// with the neighbours' stamped boundary planes in their ghost planes (U .. T address the first owned cell), and the node types of
// those two planes (tlo below the first owned plane, thi above the last; read only where the neighbour exists).  q of an own cell is
// then the single context's, bit for bit: the curl tests the GLOBAL x against the grid's faces and takes the x neighbours across a
// cut from the ghost and type planes.  A whole grid is the slab x_offset = 0, dimx = gx: both faces are the grid's, no neighbour
// exists, and tlo / thi are never read.
// VEC: what (a, b, c) is -- 0 the velocity, 1 the vorticity, 2 the invariants of the velocity gradient (div, Q, S:S; fs3d_invariants).
// Whole grids only (FS3D_OPT_OUTPUT_WALL; fs3d_wall_loads): 3 the wall shear stress tau, 4 (|tau|, q, area), on the carriers, and the
// members of a box are its carriers; 5 the velocity fields of a statistic layer of the wall sums, whose members are the cells with
// nw >= 1 that are not NODE_OUT.  What these three need rides in a base that is empty for the others: their struct is unchanged.
template <typename R, int VEC>
struct WallPart {};
template <typename R>
struct WallPart<R, 3> { WallRule<R> wall; const unsigned *nw; };
template <typename R>
struct WallPart<R, 4> : WallPart<R, 3> {};
template <typename R>
struct WallPart<R, 5> : WallPart<R, 3> {};

template <typename R, int VEC>
struct SlabCells : WallPart<R, VEC> {
    const uint16_t *code;
    const R *U, *V, *W, *T;
    const uint8_t *tlo, *thi;
    int x_offset, dimx, gx, dimy, dimz;
    R two_dx, two_dy, two_dz;
    __device__ int type_of(long long l) const { return (code[l] >> CODE_TYPE_SHIFT) & 3; }
    // (a, b, c) of the own cell l = (x, y, z), x counted from the slab's first plane, whose type is ty.  SLAB = false: no cut, the x
    // neighbours of a cell that gets this far are own cells
    template <bool SLAB = true>
    __device__ __attribute__((always_inline)) void vec_of(long long l, int x, int y, int z, int ty, R &a, R &b, R &c) const
    {
        if (VEC == 0 || VEC == 5) { a = U[l]; b = V[l]; c = W[l]; return; }
        if constexpr (VEC == 3 || VEC == 4) {
            a = b = c = ty == FS3D_NODE_OUT ? R(99999.0f) : R(0);
            member(l, x, y, z, a, b, c);
            return;
        }
        const long long plane = (long long)dimy * dimz;
        const int xg = x + x_offset;
        a = b = c = ty == FS3D_NODE_OUT ? R(99999.0f) : R(0);
        if (ty != FS3D_NODE_IN || xg < 1 || xg > gx - 2 || y < 1 || y > dimy - 2 || z < 1 || z > dimz - 2) return;
        const long long r = (long long)y * dimz + z;
        const int tm = !SLAB || x > 0 ? type_of(l - plane) : (int)tlo[r], tp = !SLAB || x < dimx - 1 ? type_of(l + plane) : (int)thi[r];
        if (tm == FS3D_NODE_OUT || tp == FS3D_NODE_OUT || type_of(l - dimz) == FS3D_NODE_OUT ||
            type_of(l + dimz) == FS3D_NODE_OUT || type_of(l - 1) == FS3D_NODE_OUT || type_of(l + 1) == FS3D_NODE_OUT) return;
        if constexpr (VEC == 1) {
            a = (W[l + dimz] - W[l - dimz]) / two_dy - (V[l + 1] - V[l - 1]) / two_dz;
            b = (U[l + 1] - U[l - 1]) / two_dz - (W[l + plane] - W[l - plane]) / two_dx;
            c = (V[l + plane] - V[l - plane]) / two_dx - (U[l + dimz] - U[l - dimz]) / two_dy;
        } else {
            const R *const F[3] = {U, V, W};
            R g[3][3];
#pragma unroll
            for (int f = 0; f < 3; f++) {
                g[f][0] = (F[f][l + plane] - F[f][l - plane]) / two_dx;
                g[f][1] = (F[f][l + dimz] - F[f][l - dimz]) / two_dy;
                g[f][2] = (F[f][l + 1] - F[f][l - 1]) / two_dz;
            }
            fs3d_invariants(g, a, b, c);
        }
    }
    // VEC >= 3: whether the own cell l = (x, y, z) is a member of its box, and then its (a, b, c); else they are left alone
    __device__ __attribute__((always_inline)) bool member(long long l, int x, int y, int z, R &a, R &b, R &c) const
    {
        if constexpr (VEC == 5) {
            if (this->nw[l] == 0u || type_of(l) == FS3D_NODE_OUT) return false;
            a = U[l]; b = V[l]; c = W[l];
            return true;
        } else if constexpr (VEC == 3 || VEC == 4) {
            R tau[3], q, area;
            if (!fs3d_wall_loads(this->wall, code, U, V, W, T, l, x, y, z, (long long)dimy * dimz, dimz, (int)code[l], tau, q, area)) return false;
            if (VEC == 3) { a = tau[0]; b = tau[1]; c = tau[2]; }
            else { a = fs3d_wall_mag(tau); b = q; c = area; }
            return true;
        } else
            return false;
    }
};

// the node types of the slab's first and last plane, a byte per cell: what the neighbours' curl reads across the cuts
__global__ void __launch_bounds__(256) k_type_planes(const uint16_t *__restrict__ code, long long plane, long long last,
                                                      uint8_t *__restrict__ first_out, uint8_t *__restrict__ last_out)
{
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < plane; r += (long long)gridDim.x * 256) {
        first_out[r] = (uint8_t)((code[r] >> CODE_TYPE_SHIFT) & 3);
        last_out[r] = (uint8_t)((code[last + r] >> CODE_TYPE_SHIFT) & 3);
    }
}

// FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR (no reference counterpart; the rule: layer_output.py): the sample (i, j, k) is the
// mean over the NODE_IN cells of its box [x0, x1) x [y0, y1) x [z0, z1) of source cells -- lo = i*g/o, hi = max(lo + 1, (i+1)*g/o) per
// axis -- and the cell (x0, y0, z0) itself where the box holds none.  `point` (filter 0 of the vorticity): every sample is that cell,
// one lane per output k as in k_get_layer, no box is walked.
// VEC 3, 4 (FS3D_OPT_OUTPUT_WALL 1, 2; whole grids): the wall loads on the carriers, and the box is averaged over its carriers in place
// of its NODE_IN cells; VEC 5 (FS3D_OPT_OUTPUT_WALL 3, 4 with the filter): the layer's values over the cells with nw >= 1.
// VEC 1: the three velocity quantities are the curl, central differences in R, on the NODE_IN cells whose six neighbours are in the
// grid and not NODE_OUT; 0 on the other NODE_IN cells and the walls, 99999 on NODE_OUT cells.  VEC 2 (FS3D_OPT_OUTPUT_GRADIENT 1):
// the invariants div, Q, S:S of the velocity gradient on the same cells, with the same values elsewhere: 18 neighbour values
// where the curl reads 12, behind the same seven codes.
// One block = one output row i and the output rows j = blockIdx.y, + gridDim.y, ...; per j the output k go in groups of 256, one
// lane per output k.  The source cells [zb, ze) under a group are walked in chunks of 256, lanes along the source k (unit stride):
// a thread runs down the planes and rows of the box for its k with four double sums and a count in registers, the per-k partials
// go through LDS and the lane of every output k adds the ones of its box.  For o <= g the boxes partition the axis, so every source
// cell is read once (2 bytes of code and four reals); no atomics, plain cached loads (the next step reads `next` again).  The curl
// reads its six neighbours through the cache (the k +- 1 ones are the neighbouring lanes' lines).  Double sums of at most 2^31
// terms; the order is the kernel's own, the rule leaves it free: per lane x outer and y inner for its source k, then the chunk's k
// ascending out of LDS, one division, one rounding.
// The rows are ia + blockIdx.x, those whose box holds a plane of this slab, and the x range of every box is clipped to the slab's
// planes.  A row whose box lies inside the slab is finished here; outV / outT address the first sample of the first OWNED row i0.
// A straddling row (its box holds planes of more than one slab; at most the first and the last row of a slab, their places in the
// group's list s_first / s_last, -1: not straddling) leaves its four double sums and its count, planar, in part[s][q][ody * odz]:
// the sums of the slabs are added over the group and k_get_layer_finish divides.  `point`: no row straddles and the rows are the
// owned ones.
// SLAB = false, the whole grid: x_offset = 0, dimx = gx, ia = i0 = 0, every row owned, none straddling, part, tlo and thi unused --
// the values the same body would run with, here known to the compiler, as k_geom_codes<SLAB> has it: the instantiation drops the
// clipping, the row offsets, the straddling store and the fetch of the type planes, and with them the 11 SGPRs that cost the
// box mean a wave per SIMD.
template <typename R, int VEC, bool SLAB>
__global__ void __launch_bounds__(256) k_get_layer_box(const SlabCells<R, VEC> s, int odx, int ody, int odz, int point, int ia, int i0,
                                                        int s_first, int s_last, R *__restrict__ outV, double *__restrict__ outT,
                                                        double *__restrict__ part)
{
    __shared__ double sq[4][256];
    __shared__ int sn[256];
    const int dimy = s.dimy, dimz = s.dimz;
    const long long plane = (long long)dimy * dimz;
    const int t = (int)threadIdx.x;
    auto box_lo = [](int i, int g, int o) { return (int)((long long)i * g / o); };
    auto box_hi = [&](int i, int lo, int g, int o) { const int h = (int)((long long)(i + 1) * g / o); return h < lo + 1 ? lo + 1 : h; };
    const int i = (SLAB ? ia : 0) + (int)blockIdx.x;
    const int sidx = !SLAB ? -1 : blockIdx.x == 0 ? s_first : blockIdx.x == gridDim.x - 1 ? s_last : -1;
    const int g0 = box_lo(i, s.gx, odx), g1 = box_hi(i, g0, s.gx, odx);
    int x0 = g0, x1 = g1;
    if constexpr (SLAB) { x0 = g0 > s.x_offset ? g0 - s.x_offset : 0; x1 = g1 - s.x_offset < s.dimx ? g1 - s.x_offset : s.dimx; }
    const long long po = (long long)ody * odz;
    for (int j = (int)blockIdx.y; j < ody; j += (int)gridDim.y) {
        const int y0 = box_lo(j, dimy, ody), y1 = box_hi(j, y0, dimy, ody);
        for (long long kg = 0; kg < odz; kg += 256) {          // (64-bit: odz may lie within 256 of 2^31)
            const int klast = (int)(kg + 256 < odz ? kg + 256 : odz) - 1;
            const bool kout = kg + t < odz;
            const int ko = kout ? (int)kg + t : klast;
            const int z0 = box_lo(ko, dimz, odz), z1 = box_hi(ko, z0, dimz, odz);
            // the group's source cells, block-uniform; `point`: none are walked, every lane takes the one cell of its own output k below
            const int zb = box_lo((int)kg, dimz, odz), zl = box_lo(klast, dimz, odz), ze = point ? zb : box_hi(klast, zl, dimz, odz);
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            int n = 0;
            for (int cb = zb; cb < ze; cb += 256) {
                const int z = cb + t;
                double q[4] = {0.0, 0.0, 0.0, 0.0};
                int m = 0;
                if (z < ze)
                    for (int x = x0; x < x1; x++)
                        for (int y = y0; y < y1; y++) {
                            const long long l = (long long)x * plane + (long long)y * dimz + z;
                            R a, b, c;
                            if constexpr (VEC >= 3) {                  // the wall records: the members are not the fluid cells
                                if (!s.member(l, x, y, z, a, b, c)) continue;
                            } else {
                                if (s.type_of(l) != FS3D_NODE_IN) continue;
                                s.template vec_of<SLAB>(l, x, y, z, FS3D_NODE_IN, a, b, c);
                            }
                            q[0] += (double)a; q[1] += (double)b; q[2] += (double)c; q[3] += (double)s.T[l];
                            m++;
                        }
#pragma unroll
                for (int v = 0; v < 4; v++) sq[v][t] = q[v];
                sn[t] = m;
                __syncthreads();
                if (kout) {
                    const int e = z1 < cb + 256 ? z1 : cb + 256;
                    for (int zz = z0 > cb ? z0 : cb; zz < e; zz++) {
#pragma unroll
                        for (int v = 0; v < 4; v++) acc[v] += sq[v][zz - cb];
                        n += sn[zz - cb];
                    }
                }
                __syncthreads();
            }
            if (!kout) continue;
            if (SLAB && sidx >= 0) {                                   // the group adds the slabs' sums; the row's owner finishes
                double *const p = part + (long long)sidx * 5 * po + (long long)j * odz + ko;
#pragma unroll
                for (int v = 0; v < 4; v++) p[v * po] = acc[v];
                p[4 * po] = (double)n;
                continue;
            }
            const long long ind = ((long long)(i - (SLAB ? i0 : 0)) * ody + j) * odz + ko;
            if (n) {
                const double d = (double)n;
                outV[3 * ind] = (R)(acc[0] / d); outV[3 * ind + 1] = (R)(acc[1] / d); outV[3 * ind + 2] = (R)(acc[2] / d);
                outT[ind] = acc[3] / d;
            } else {                                           // no fluid in the box, or `point`: the point sample (on a wall, or the stamp);
                                                               // the box is inside the slab: so is its first cell
                const long long l = (long long)x0 * plane + (long long)y0 * dimz + z0;
                R a, b, c;
                s.template vec_of<SLAB>(l, x0, y0, z0, s.type_of(l), a, b, c);
                outV[3 * ind] = a; outV[3 * ind + 1] = b; outV[3 * ind + 2] = c;
                outT[ind] = (double)s.T[l];
            }
        }
    }
}

// The owner of the straddling row i (the slab that holds the first plane of its box) finishes it from the group's sums: one
// division and one rounding per quantity, or the point sample of the cell (lo_x, lo_y, lo_z) where no slab counted a NODE_IN cell.
// One thread per sample, k fastest; `part` addresses the row's five planes, outV / outT the row's first sample.
template <typename R, int VEC>
__global__ void __launch_bounds__(256) k_get_layer_finish(const SlabCells<R, VEC> s, int i, int odx, int ody, int odz,
                                                           const double *__restrict__ part, R *__restrict__ outV, double *__restrict__ outT)
{
    const long long po = (long long)ody * odz;
    const long long plane = (long long)s.dimy * s.dimz;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < po; p += (long long)gridDim.x * 256) {
        const double d = part[4 * po + p];
        if (d > 0.0) {
            outV[3 * p] = (R)(part[p] / d); outV[3 * p + 1] = (R)(part[po + p] / d); outV[3 * p + 2] = (R)(part[2 * po + p] / d);
            outT[p] = part[3 * po + p] / d;
        } else {
            const int j = (int)(p / odz), k = (int)(p - (long long)j * odz);
            const int x = (int)((long long)i * s.gx / odx) - s.x_offset, y = (int)((long long)j * s.dimy / ody), z = (int)((long long)k * s.dimz / odz);
            const long long l = (long long)x * plane + (long long)y * s.dimz + z;
            R a, b, c;
            s.vec_of(l, x, y, z, s.type_of(l), a, b, c);
            outV[3 * p] = a; outV[3 * p + 1] = b; outV[3 * p + 2] = c;
            outT[p] = (double)s.T[l];
        }
    }
}

// FS3D_OPT_OUTPUT_SLABS: (x_offset, dimx) of every rank into os_cuts, one all-gather per context (8 bytes per rank: two ints, moved
// as elements of the context's precision).  The slabs must be the group's partition of [0, dimx_global) in rank order.
static fs3d_status gather_cuts(fs3d_ctx *c)
{
    const int nr = c->nranks;
    BUFCHK(c, c->os_cut_dev.reserve((size_t)(nr + 1) * 8));
    int *const dev = (int *)c->os_cut_dev.raw();
    const int mine[2] = {c->x_offset, c->dimx};
    HIPCHK(c, hipMemcpyAsync(dev + 2 * nr, mine, sizeof mine, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                // `mine` is pageable: the copy has left it
    GTRY(fs3d_comm_allgather(c, dev + 2 * nr, dev, 8 / c->esize));
    std::vector<int> cuts((size_t)2 * nr);
    HIPCHK(c, hipMemcpyAsync(cuts.data(), dev, (size_t)nr * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int at = 0;
    for (int r = 0; r < nr; r++) {
        if (cuts[2 * r] != at || cuts[2 * r + 1] < 1) return fail(c, FS3D_ERR_INVALID, "FS3D_OPT_OUTPUT_SLABS: the slabs of the group do not partition the grid's planes in rank order");
        at += cuts[2 * r + 1];
    }
    if (at != c->dimx_global) return fail(c, FS3D_ERR_INVALID, "FS3D_OPT_OUTPUT_SLABS: the slabs of the group do not partition the grid's planes in rank order");
    c->os_cuts = cuts;
    return FS3D_OK;
}

// Solver3D::GetLayer, Solver3D.cpp:21-25: next->Clear(NODE_OUT, MISSING_VALUE), then FilterToArrays by k_get_layer.
// `local`: the slab's own planes are the whole source (fs3d_get_layer: x = i*dimx/odx, rows [0, odx)); else the slab owns the rows
// of the GLOBAL output whose source plane it holds.  `dev`: outV / outT are on the context's device, the kernel writes them and
// the call returns after the enqueue; else the owned samples go through the staging buffer and the call returns synchronised.
// One sequence for every record: the rows -- the source layer -- the stamp -- the record stage -- the copies.
// FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR: the record stage is k_get_layer_box in place of k_get_layer.
// FS3D_OPT_OUTPUT_GRADIENT 1: the same stage with VEC = 2, the invariants where the vector option has the curl -- "the vector option"
// below stands for either.  FS3D_OPT_OUTPUT_GRADIENT 2 (with source 1): k_time_grad_layer of kernels_stats.hip writes the mean
// invariants over U, V, W of the statistic layer, which is then sampled as a velocity layer (VEC = 0).
// FS3D_OPT_OUTPUT_SOURCE 1..3 (source 2: the layer FS3D_OPT_OUTPUT_MOMENT chooses): the statistic layer of kernels_stats.hip, in a
// buffer of its own, takes the place of `next` -- stamp, record stage, staging and copies run on it unchanged; `next` and `cur` are
// not written.
// `collective` (FS3D_OPT_OUTPUT_SLABS on a member of a group, with the filter or the vector option set): the record as ONE
// COLLECTIVE call, and the only form that reaches fs3d_comm.h.  Every rank runs the same sequence whatever it owns; what the flag
// adds: (the cuts, once) and from them the straddling rows, which every rank finds alike -- with the vector option one grouped
// exchange of the sampled layer's boundary planes and the type planes -- with at least one straddling row one all-reduce of their
// partial sums, and k_get_layer_finish on the straddling row the rank owns.  A record that is not collective is the same stage with
// an empty list.  The `dev` form of a collective record may synchronise in the transport; the caller aborts the group when a
// collective record fails.
template <typename R>
static fs3d_status get_layer_impl(fs3d_ctx *c, R *outV, double *outT, int odx, int ody, int odz, bool local, bool dev, bool collective, int rows[2])
{
    const int b = c->slot[FS3D_LAYER_NEXT];
    const int gx = local ? c->dimx : c->dimx_global, x_offset = local ? 0 : c->x_offset;
    if (odx == 0) odx = gx;
    if (ody == 0) ody = c->dimy;
    if (odz == 0) odz = c->dimz;
    const long long po = (long long)ody * odz;
    if (po >= (1LL << 31)) return fail(c, FS3D_ERR_UNSUPPORTED, "fs3d_get_layer: an output plane of 2^31 samples or more");
    // SlabCells' VEC (the three options exclude each other); the time means of the wall loads are a velocity layer, with members
    // of their own under the filter
    const int vec = c->opt_out_wall == 1 ? 3 : c->opt_out_wall == 2 ? 4 : c->opt_out_wall && c->opt_out_filter ? 5 : c->opt_out_gradient == 1 ? 2 : c->opt_out_vector;
    // the rows i with x_offset <= i*gx/odx < x_offset + dimx (slab.py out_rows)
    const int i0 = (int)(((long long)x_offset * odx + gx - 1) / gx), i1 = (int)(((long long)(x_offset + c->dimx) * odx + gx - 1) / gx);
    if (rows) { rows[0] = i0; rows[1] = i1; }
    const long long n = (long long)(i1 - i0) * po;
    const size_t vbytes = ((size_t)3 * n * sizeof(R) + 255) / 256 * 256;
    c->gl_info[0] = n; c->gl_info[1] = 0;
    R *dV = outV + 3 * (size_t)i0 * po;
    double *dT = outT + (size_t)i0 * po;
    // the straddling rows: per cut the row whose box begins below it, where that box reaches beyond it (the box mean only: a point
    // sample is one cell).  Ascending, a row over several cuts once; the same list on every rank
    auto box_lo = [](int i, int g, int o) { return (int)((long long)i * g / o); };
    auto box_hi = [&](int i, int g, int o) { return std::max(box_lo(i, g, o) + 1, (int)((long long)(i + 1) * g / o)); };
    std::vector<int> list;
    if (collective) {
        if (c->os_cuts.empty()) GTRY(gather_cuts(c));
        if (c->opt_out_filter)
            for (int r = 1; r < c->nranks; r++) {
                const int cut = c->os_cuts[2 * r], i = (int)(((long long)cut * odx + gx - 1) / gx) - 1;
                if (i >= 0 && box_lo(i, gx, odx) < cut && box_hi(i, gx, odx) > cut && (list.empty() || list.back() != i)) list.push_back(i);
            }
    }
    auto place = [&](int i) { const auto it = std::find(list.begin(), list.end(), i); return it == list.end() ? -1 : (int)(it - list.begin()); };
    // the rows this slab's planes take part in: the owned ones, and in front of them the row that begins in a slab below
    const int ia = i0 > 0 && place(i0 - 1) >= 0 && box_hi(i0 - 1, gx, odx) > x_offset ? i0 - 1 : i0;
    const int s_first = i1 > ia ? place(ia) : -1, s_last = i1 > ia ? place(i1 - 1) : -1;
    const bool finish = i1 > i0 && s_last >= 0;              // the last owned row reaches into the next slab
    const size_t nsum = list.size() * (size_t)5 * po;
    // gl_info[2] counts every allocation once: a reserve only ever sets its flag, so each gets a flag of its own
    if (!dev && n) { bool grown = false; BUFCHK(c, c->gl_stage.reserve(vbytes + (size_t)n * 8, nullptr, &grown)); c->gl_info[2] += grown; }
    if (collective && vec) { bool grown = false; BUFCHK(c, c->os_type.reserve((size_t)4 * c->plane, nullptr, &grown)); c->gl_info[2] += grown; }
    if (nsum) { bool grown = false; BUFCHK(c, c->os_part.reserve(nsum * sizeof(double), nullptr, &grown)); c->gl_info[2] += grown; }
    R *F[4] = {fld<R>(c, b, 0), fld<R>(c, b, 1), fld<R>(c, b, 2), fld<R>(c, b, 3)};
    long long fstride = c->fstride;
    if (c->opt_out_source) {                                   // a collective record exchanges the layer's ghost planes: it asks for them
        bool grown = false;
        GTRY(fs3d_time_stats_layer(c, c->opt_out_source, c->opt_out_source == 2 ? c->opt_out_moment : 0, (void **)F, &grown, collective, &fstride));
        c->gl_info[2] += grown;
        if (c->opt_out_gradient == 2) GTRY(fs3d_time_stats_grad_layer(c, F[0], fstride));      // U, V, W of the mean layer: the mean invariants
        if (c->opt_out_wall >= 3) GTRY(fs3d_time_stats_wall_layer(c, c->opt_out_wall, F[0], fstride));      // ... the mean wall loads
    }
    hipLaunchKernelGGL((k_clear_type<R>), dim3(grid_for(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell,
                       (int)FS3D_NODE_OUT, (R)99999.0f, F[0], F[1], F[2], F[3]);
    HIPCHK(c, hipGetLastError());
    uint8_t *const ty = c->os_type;
    if (collective && vec) {
        hipLaunchKernelGGL(k_type_planes, dim3(grid_for(c->plane)), dim3(256), 0, c->stream, (const uint16_t *)c->code, c->plane,
                           (long long)(c->dimx - 1) * c->plane, ty, ty + c->plane);
        HIPCHK(c, hipGetLastError());
        GTRY(fs3d_comm_layer_exchange(c, F[0] - c->plane, fstride, {ty, ty + c->plane, ty + 2 * c->plane, ty + 3 * c->plane}));
    }
    if (nsum) HIPCHK(c, hipMemsetAsync(c->os_part, 0, nsum * sizeof(double), c->stream));
    R *kV = dev ? dV : (R *)c->gl_stage;
    double *kT = dev ? dT : (double *)((char *)c->gl_stage + vbytes);
    auto box_stage = [&](auto vec_c) {
        constexpr int VEC = decltype(vec_c)::value;
        // not collective: the whole grid.  No neighbour exists and the two type planes are null; they would never be read -- a cell on
        // the grid's first or last plane returns from SlabCells::vec_of before the neighbour types are fetched -- and SLAB = false
        // compiles the fetch out
        const bool cut_types = collective && VEC != 0;
        SlabCells<R, VEC> s{{}, c->code, F[0], F[1], F[2], F[3], cut_types ? ty + 2 * c->plane : nullptr, cut_types ? ty + 3 * c->plane : nullptr,
                             x_offset, c->dimx, gx, c->dimy, c->dimz, R(2) * (R)c->gdx, R(2) * (R)c->gdy, R(2) * (R)c->gdz};
        if constexpr (VEC >= 3) { s.wall = fs3d_wall_rule<R>(c->gdx, c->gdy, c->gdz, c->v_vis, c->t_vis); s.nw = c->tw_n; }
        if (i1 > ia) {
            auto launch = [&](auto slab) {
                hipLaunchKernelGGL((k_get_layer_box<R, VEC, decltype(slab)::value>), dim3((unsigned)(i1 - ia), (unsigned)std::min(ody, 65535)), dim3(256), 0, c->stream, s,
                                   odx, ody, odz, c->opt_out_filter ? 0 : 1, ia, i0, s_first, s_last, kV, kT, (double *)c->os_part);
            };
            if constexpr (VEC >= 3) launch(std::false_type{});          // the wall records: whole grids only, the entries refuse a slab
            else if (collective) launch(std::true_type{}); else launch(std::false_type{});
        }
        if (const hipError_t e = hipGetLastError(); e != hipSuccess)       // (checked where no row is launched too, as ever)
            return fail(c, FS3D_ERR_HIP, collective ? call_failed(c, "k_get_layer_box", "launch") : call_failed(c, "hipGetLastError()", hipGetErrorString(e)));
        if (nsum) GTRY(fs3d_comm_allreduce_sum(c, c->os_part, nsum));
        if constexpr (VEC < 3) if (finish) {
            const long long at = (long long)(i1 - 1 - i0) * po;
            hipLaunchKernelGGL((k_get_layer_finish<R, VEC>), dim3(grid_for(po, 1024)), dim3(256), 0, c->stream, s, i1 - 1, odx, ody, odz,
                               (const double *)c->os_part + (size_t)s_last * 5 * po, kV + 3 * at, kT + at);
            if (hipGetLastError() != hipSuccess) return fail(c, FS3D_ERR_HIP, call_failed(c, "k_get_layer_finish", "launch"));
        }
        return FS3D_OK;
    };
    if (c->opt_out_filter || vec)
        GTRY(vec == 5 ? box_stage(std::integral_constant<int, 5>{}) : vec == 4 ? box_stage(std::integral_constant<int, 4>{}) : vec == 3 ? box_stage(std::integral_constant<int, 3>{})
             : vec == 2 ? box_stage(std::integral_constant<int, 2>{}) : vec ? box_stage(std::integral_constant<int, 1>{}) : box_stage(std::integral_constant<int, 0>{}));
    else if (n) {
        hipLaunchKernelGGL((k_get_layer<R>), dim3((unsigned)(i1 - i0), grid_for(po, 1024)), dim3(256), 0, c->stream, F[0], F[1], F[2], F[3],
                           x_offset, c->dimx, c->plane, c->dimy, c->dimz, gx, odx, ody, odz, i0, i1, kV, kT);
        HIPCHK(c, hipGetLastError());
    }
    if (!dev && n) {
        HIPCHK(c, hipMemcpyAsync(dV, kV, (size_t)3 * n * sizeof(R), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(dT, kT, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        c->gl_info[1] = n * (long long)(3 * sizeof(R) + 8);
    }
    if (dev) return FS3D_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->ev_used) rec_collect(c);
    return check_device_errors(c);
}

// the three output entries: refusals before any launch, then the precision's get_layer_impl
static fs3d_status get_layer_entry(fs3d_ctx *c, const char *what, void *outV, double *outT, int odx, int ody, int odz, bool local, bool dev, int rows[2])
{
    if (!c || !outV || !outT || (!local && !rows)) return c ? fail(c, FS3D_ERR_INVALID, std::string(what) + ": NULL destination") : FS3D_ERR_INVALID;
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, std::string(what) + ": upload nodes first");
    if (odx < 0 || ody < 0 || odz < 0) return fail(c, FS3D_ERR_INVALID, std::string(what) + ": negative output dims");
    if (c->opt_out_wall) {                                     // FS3D_OPT_OUTPUT_WALL: whole grids only, and outV is its own
        const std::string w = std::string(what) + ": FS3D_OPT_OUTPUT_WALL " + std::to_string(c->opt_out_wall);
        if (c->opt_out_vector || c->opt_out_gradient)
            return fail(c, FS3D_ERR_INVALID, w + (c->opt_out_vector ? " with FS3D_OPT_OUTPUT_VECTOR 1" : " with FS3D_OPT_OUTPUT_GRADIENT set") + " (two options claim outV)");
        if (c->opt_out_source >= 2)
            return fail(c, FS3D_ERR_INVALID, w + " with FS3D_OPT_OUTPUT_SOURCE " + std::to_string(c->opt_out_source) + " (the wall loads of a variance or a fraction layer mean nothing)");
        if (c->x_offset != 0 || c->dimx != c->dimx_global || c->comm || c->local || c->nranks > 1)
            return fail(c, FS3D_ERR_UNSUPPORTED, w + " on an x-slab or a member of a group (the faces across a cut need the neighbour's planes; FS3D_OPT_OUTPUT_SLABS does not serve it)");
        if (c->opt_out_wall >= 3 && (c->opt_out_source != 1 || c->opt_time_stats == 0 || !c->opt_ts_wall || c->ts_steps == 0 || !c->tw_n.raw() || !c->tw_w.raw()))
            return fail(c, FS3D_ERR_INVALID, w + " asks for a time mean of the wall loads: it needs FS3D_OPT_OUTPUT_SOURCE 1 and an open window of "
                                             "FS3D_OPT_TIME_STATS with FS3D_OPT_TIME_STATS_WALL 1 that holds a time step");
    }
    if (c->opt_out_gradient && c->opt_out_vector)
        return fail(c, FS3D_ERR_INVALID, std::string(what) + ": FS3D_OPT_OUTPUT_GRADIENT " + std::to_string(c->opt_out_gradient) +
                                         " with FS3D_OPT_OUTPUT_VECTOR 1 (two options claim outV)");
    if (c->opt_out_gradient == 2 && (c->opt_out_source != 1 || c->opt_time_stats == 0 || !c->opt_ts_grad || c->ts_steps == 0 || !c->tg_n.raw() || !c->tg_g.raw()))
        return fail(c, FS3D_ERR_INVALID, std::string(what) + ": FS3D_OPT_OUTPUT_GRADIENT 2 asks for the time mean of the invariants: it needs FS3D_OPT_OUTPUT_SOURCE 1 and an "
                                         "open window of FS3D_OPT_TIME_STATS with FS3D_OPT_TIME_STATS_GRAD 1 that holds a time step");
    const bool slab_record = (c->opt_out_filter || c->opt_out_vector || c->opt_out_gradient == 1) &&
                             (c->x_offset != 0 || c->dimx != c->dimx_global || c->comm || c->local || c->nranks > 1);
    if (slab_record && !c->opt_out_slabs)
        return fail(c, FS3D_ERR_UNSUPPORTED, std::string(what) + ": FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR / FS3D_OPT_OUTPUT_GRADIENT on an x-slab or a member of a group "
                                             "(a box can straddle a cut, the curl and the gradient need the neighbour's planes)");
    if (slab_record && local)
        return fail(c, FS3D_ERR_UNSUPPORTED, std::string(what) + ": FS3D_OPT_OUTPUT_FILTER / FS3D_OPT_OUTPUT_VECTOR / FS3D_OPT_OUTPUT_GRADIENT on an x-slab: this entry samples the slab's own "
                                             "planes and is not collective; FS3D_OPT_OUTPUT_SLABS serves fs3d_get_layer_rows and fs3d_get_layer_dev");
    if (slab_record && !c->comm && !c->local)
        return fail(c, FS3D_ERR_UNSUPPORTED, std::string(what) + ": FS3D_OPT_OUTPUT_SLABS: a lone x-slab of a larger grid needs its neighbours' planes and sums: "
                                             "make it a member of a group (fs3d_comm_init_local, fs3d_comm_init) first");
    if (c->opt_out_source) {
        const char *const names[4] = {"", "the time mean", "the time variance", "the fluid fraction"};
        if (c->opt_time_stats == 0 || (c->opt_out_source == 2 && c->opt_time_stats < 2))
            return fail(c, FS3D_ERR_INVALID, std::string(what) + ": FS3D_OPT_OUTPUT_SOURCE asks for " + names[c->opt_out_source] +
                                             ", which the FS3D_OPT_TIME_STATS mode " + std::to_string(c->opt_time_stats) + " does not hold");
        if (c->opt_out_source == 2 && c->opt_out_moment) {         // the moment is read for source 2 only
            if (c->opt_time_stats < 2 || !c->opt_ts_cross)
                return fail(c, FS3D_ERR_INVALID, std::string(what) + ": FS3D_OPT_OUTPUT_MOMENT " + std::to_string(c->opt_out_moment) +
                                                 " asks for covariances, and the open window holds no cross sums (FS3D_OPT_TIME_STATS 2 with FS3D_OPT_TIME_STATS_CROSS 1)");
            if (c->opt_out_vector || c->opt_out_gradient == 1)
                return fail(c, FS3D_ERR_INVALID, std::string(what) + ": FS3D_OPT_OUTPUT_MOMENT " + std::to_string(c->opt_out_moment) +
                                                 (c->opt_out_vector ? " with FS3D_OPT_OUTPUT_VECTOR 1 (the curl of a stress layer means nothing)"
                                                                    : " with FS3D_OPT_OUTPUT_GRADIENT 1 (the gradient of a stress layer means nothing)"));
        }
        if (c->ts_steps == 0) return fail(c, FS3D_ERR_INVALID, std::string(what) + ": the window of FS3D_OPT_TIME_STATS holds no time step yet");
    }
    HIPCHK(c, hipSetDevice(c->device));
    auto run = [&]() { return c->prec == FS3D_F32 ? get_layer_impl<float>(c, (float *)outV, outT, odx, ody, odz, local, dev, slab_record, rows)
                                                  : get_layer_impl<double>(c, (double *)outV, outT, odx, ody, odz, local, dev, slab_record, rows); };
    if (!slab_record) return run();
    fs3d_status st = FS3D_ERR_HIP;                             // collective from here on: a rank that fails takes the group down
    AbortOnError guard{c, &st};
    return st = run();
}

extern "C" fs3d_status fs3d_get_layer(fs3d_ctx *c, void *outV, double *outT, int odx, int ody, int odz)
{
    return get_layer_entry(c, "fs3d_get_layer", outV, outT, odx, ody, odz, true, false, nullptr);
}

extern "C" fs3d_status fs3d_get_layer_rows(fs3d_ctx *c, void *outV, double *outT, int odx, int ody, int odz, int rows[2])
{
    return get_layer_entry(c, "fs3d_get_layer_rows", outV, outT, odx, ody, odz, false, false, rows);
}

extern "C" fs3d_status fs3d_get_layer_dev(fs3d_ctx *c, void *outV, double *outT, int odx, int ody, int odz, int rows[2])
{
    return get_layer_entry(c, "fs3d_get_layer_dev", outV, outT, odx, ody, odz, false, true, rows);
}

extern "C" fs3d_status fs3d_get_layer_info(fs3d_ctx *c, long long info[FS3D_N_GETLAYER_INFO])
{
    if (!c || !info) return FS3D_ERR_INVALID;
    for (int k = 0; k < FS3D_N_GETLAYER_INFO; k++) info[k] = c->gl_info[k];
    return FS3D_OK;
}
