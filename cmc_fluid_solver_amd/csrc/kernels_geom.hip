// Moving geometry: the tables the sweeps read, rebuilt on the device between time steps
// (fs3d_update_nodes / fs3d_update_nodes_dev), Solver3D::ClearOutterCells (fs3d_clear_outer_cells) and the
// table summary fs3d_geometry_info.  The host routine upload_nodes_impl (fs3d_hip.hip) stays the first upload and the
// definition of every table; the kernels here end with the same tables.
// Also the extrusion of a Shape2D grid into the node arrays on the device (k_geom_extrude; fs3d_extrude_shape2d_dev,
// fs3d_update_nodes_shape2d): a moving Shape2D geometry then ships its 2D grid per step, not the 3D node arrays.
//
// Row kinds without the serial walk of line_kinds (fs3d_hip.hip): that walk opens a run at `pos` when cell pos + 1 is
// NODE_IN and closes it at the first cell after the run that is not NODE_IN; a run that reaches the end of the line is
// dropped.  So, with Lst = the last index of the line whose type is not NODE_IN (-1: none),
//   INTERIOR(s)  <=>  s >= 1, type[s] == NODE_IN and s < Lst        (cell 0 only ever opens a run; s < Lst: a closing cell exists)
//   START(s)     <=>  !INTERIOR(s) and INTERIOR(s + 1)
//   END(s)       <=>  !INTERIOR(s) and INTERIOR(s - 1)
// where the walk lets START overwrite END on a cell that closes one run and opens the next (the cell of the shared-FREE
// refusal), and the number of segments is the number of START cells.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>

#include "fs3d_common.h"

static fs3d_status gfail(fs3d_ctx *c, fs3d_status st, const std::string &msg)
{
    if (c) c->err = msg;
    return st;
}

#define GHIP(c, call)                                                                                \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            char b_[512];                                                                            \
            snprintf(b_, sizeof b_, "GPU %d: %s failed: %s", (c)->device, #call, hipGetErrorString(e_)); \
            return gfail((c), FS3D_ERR_HIP, b_);                                                     \
        }                                                                                            \
    } while (0)

// device allocations / frees of the geometry paths are counted (fs3d_geometry_info entry 13)
#define GMALLOC(c, pp, bytes) do { GHIP(c, hipMalloc((void **)(pp), (bytes))); (c)->geom_allocs++; } while (0)
static void gfree(fs3d_ctx *c, void *p) { if (p) { hipFree(p); c->geom_allocs++; } }

// counter words of one update (device, read back once)
enum { GC_NSEG = 0 /* 0..2 */, GC_NBND = 3, GC_STALE = 4, GC_SHARED = 5, GC_LIST = 6, GC_MISMATCH = 7, GC_WORDS = 8 };

// ---------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------

// X and Y lines: cells `ss` apart, neighbouring lines along k contiguous -- one thread per line, lanes along k read coalesced.
// lst[line] = last index whose type is not NODE_IN (-1: none); dead[line] = 1 when the line has no NODE_IN cell (every cell on a
// segment lies on a line with a NODE_IN cell, so this is upload_nodes_impl's "no segment cell and no NODE_IN cell").
__global__ void __launch_bounds__(256) k_geom_lines_strided(const uint8_t *__restrict__ type, int n_o, int dimz, long long os,
                                                             long long ss, int n, int *__restrict__ lst, uint8_t *__restrict__ dead)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_o * dimz) return;
    const int o = (int)(t / dimz), k = (int)(t - (long long)o * dimz);
    const uint8_t *p = type + (long long)o * os + k;
    int last = -1, any_in = 0;
    for (int s = 0; s < n; s++) {
        if (p[(long long)s * ss] != FS3D_NODE_IN) last = s; else any_in = 1;
    }
    lst[t] = last;
    dead[t] = any_in ? 0 : 1;
}

// Z lines are the contiguous axis: one wave per line, lanes along the line
__global__ void __launch_bounds__(256) k_geom_lines_z(const uint8_t *__restrict__ type, long long nlines, int dimz,
                                                       int *__restrict__ lst, uint8_t *__restrict__ dead)
{
    const long long line = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (line >= nlines) return;                       // whole waves leave together
    const uint8_t *p = type + line * dimz;
    int last = -1, any_in = 0;
    for (int k = lane; k < dimz; k += 64) {
        if (p[k] != FS3D_NODE_IN) last = k; else any_in = 1;
    }
    for (int off = 32; off > 0; off >>= 1) {
        last = max(last, __shfl_xor(last, off, 64));
        any_in |= __shfl_xor(any_in, off, 64);
    }
    if (lane == 0) { lst[line] = last; dead[line] = any_in ? 0 : 1; }
}

__device__ __forceinline__ bool geom_interior(int s, int ty, int lst) { return s >= 1 && ty == FS3D_NODE_IN && s < lst; }

// row code of one direction for the cell at index s of its line (n cells); *shared: the cell closes one segment and opens the next
__device__ __forceinline__ int geom_row_code(int s, int n, int t0, int tm, int tp, int lst, int bits, bool *shared)
{
    const bool in0 = geom_interior(s, t0, lst);
    const bool inm = s >= 1 && geom_interior(s - 1, tm, lst);
    const bool inp = s + 1 < n && geom_interior(s + 1, tp, lst);
    *shared = !in0 && inm && inp;
    if (in0) return ROW_INTERIOR;
    if (inp) return ROW_START | bits;
    if (inm) return ROW_END | bits;
    return ROW_SKIP;
}

// The cell codes of all three directions in one pass, with the counts the host needs: START cells per direction (= segments),
// BOUND / VALVE cells, NODE_IN cells on no segment of a direction (stale_in_cells), shared cells that carry a FREE condition.
__global__ void __launch_bounds__(256) k_geom_codes(const uint8_t *__restrict__ type, const uint8_t *__restrict__ bc_vel,
                                                     const uint8_t *__restrict__ bc_temp, const int *__restrict__ lstx,
                                                     const int *__restrict__ lsty, const int *__restrict__ lstz, int dimx, int dimy,
                                                     int dimz, uint16_t *__restrict__ code, unsigned long long *cnt)
{
    const long long plane = (long long)dimy * dimz, ncell = plane * dimx;
    unsigned acc[6] = {0, 0, 0, 0, 0, 0};
    for (long long l = (long long)blockIdx.x * 256 + threadIdx.x; l < ncell; l += (long long)gridDim.x * 256) {
        const int i = (int)(l / plane), rem = (int)(l - (long long)i * plane), j = rem / dimz, k = rem - j * dimz;
        const int t0 = type[l];
        int bits = 0;
        if (bc_vel[l] == FS3D_BC_FREE) bits |= ROW_VELFREE;
        if (bc_temp[l] == FS3D_BC_FREE) bits |= ROW_TEMPFREE;
        bool sh[3];
        const int rx = geom_row_code(i, dimx, t0, i >= 1 ? type[l - plane] : 0, i + 1 < dimx ? type[l + plane] : 0,
                                     lstx[rem], bits, &sh[0]);
        const int ry = geom_row_code(j, dimy, t0, j >= 1 ? type[l - dimz] : 0, j + 1 < dimy ? type[l + dimz] : 0,
                                     lsty[(long long)i * dimz + k], bits, &sh[1]);
        const int rz = geom_row_code(k, dimz, t0, k >= 1 ? type[l - 1] : 0, k + 1 < dimz ? type[l + 1] : 0,
                                     lstz[(long long)i * dimy + j], bits, &sh[2]);
        code[l] = (uint16_t)(rx | (ry << 4) | (rz << 8) | ((t0 & 3) << CODE_TYPE_SHIFT));
        acc[0] += (rx & 3) == ROW_START; acc[1] += (ry & 3) == ROW_START; acc[2] += (rz & 3) == ROW_START;
        acc[3] += t0 == FS3D_NODE_BOUND || t0 == FS3D_NODE_VALVE;
        if (t0 == FS3D_NODE_IN) acc[4] += ((rx & 3) == ROW_SKIP) + ((ry & 3) == ROW_SKIP) + ((rz & 3) == ROW_SKIP);
        acc[5] += (sh[0] || sh[1] || sh[2]) && bits != 0;
    }
    __shared__ unsigned s_acc[6];
    if (threadIdx.x < 6) s_acc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 6; q++) {
        unsigned v = acc[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_acc[q], v);
    }
    __syncthreads();
    if (threadIdx.x < 6 && s_acc[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)s_acc[threadIdx.x]);
}

// Compact list of the BOUND / VALVE cells and their node values (k_impose_list reads it): wave ballots, ONE atomic per workgroup
// and tile of 2048 cells (one per wave was two thirds of the whole update on a grid with many wall cells: 262 144 returning atomics
// on one address at 256^3).  The order of the list is free: every index appears once.
#define GEOM_LIST_CHUNKS 8
template <typename R>
__global__ void __launch_bounds__(256) k_geom_bnd_list(const uint8_t *__restrict__ type, long long ncell, const R *__restrict__ node,
                                                        long long nstride, int cap, int *__restrict__ idx, R *v0, R *v1, R *v2, R *v3,
                                                        unsigned long long *cnt)
{
    __shared__ unsigned s_cnt[4];
    __shared__ unsigned long long s_first;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long tile_cells = 256LL * GEOM_LIST_CHUNKS;
    for (long long tile = (long long)blockIdx.x * tile_cells; tile < ncell; tile += (long long)gridDim.x * tile_cells) {   // workgroup-uniform
        unsigned long long m[GEOM_LIST_CHUNKS];
        unsigned tot = 0;
#pragma unroll
        for (int q = 0; q < GEOM_LIST_CHUNKS; q++) {
            const long long l = tile + (long long)(w * GEOM_LIST_CHUNKS + q) * 64 + lane;
            const int t0 = l < ncell ? type[l] : FS3D_NODE_OUT;
            m[q] = __ballot(t0 == FS3D_NODE_BOUND || t0 == FS3D_NODE_VALVE);
            tot += __popcll(m[q]);
        }
        if (lane == 0) s_cnt[w] = tot;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned all = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_first = all ? atomicAdd(&cnt[GC_LIST], (unsigned long long)all) : 0ull;
        }
        __syncthreads();
        long long pos = (long long)s_first;
        for (int ww = 0; ww < w; ww++) pos += s_cnt[ww];
#pragma unroll
        for (int q = 0; q < GEOM_LIST_CHUNKS; q++) {
            if ((m[q] >> lane) & 1) {
                const long long l = tile + (long long)(w * GEOM_LIST_CHUNKS + q) * 64 + lane;
                const long long at = pos + __popcll(m[q] & ((1ull << lane) - 1));
                if (at < cap) {
                    idx[at] = (int)l;
                    v0[at] = node[l]; v1[at] = node[nstride + l]; v2[at] = node[2 * nstride + l]; v3[at] = node[3 * nstride + l];
                }
            }
            pos += __popcll(m[q]);
        }
        __syncthreads();                                             // s_cnt / s_first are rewritten by the next tile
    }
}

__device__ __forceinline__ unsigned long long geom_mix(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Shared code columns of direction d (X: o = j, cells along i; Y: o = i, cells along j), as upload_nodes_impl defines them: one
// wave per pair of groups (g, g + 1) of 32 neighbouring lines, lanes 0..31 the lines of g, lanes 32..63 those of g + 1.
// col[o][g][s] = the (row code of d, node type) of the group's first live line; cflag bit 0 = every live line of the group equals
// it on every cell, bit 1 (even g) = so does the pair; hash[o][g] = a hash of the column for the host's identity decision.
__global__ void __launch_bounds__(64) k_geom_columns(const uint16_t *__restrict__ code, const uint8_t *__restrict__ dead, int ng,
                                                      int dimz, long long os, long long ss, int n, int keep, uint16_t *col,
                                                      uint8_t *__restrict__ cflag, unsigned long long *__restrict__ hash)
{
    const int npair = (ng + 1) / 2;
    const int o = blockIdx.x / npair, g0 = 2 * (blockIdx.x % npair);
    const int lane = threadIdx.x, half = lane >> 5;
    const int g = g0 + half, k = 32 * g + (lane & 31);
    const bool have_g = g < ng;
    const bool live = have_g && k < dimz && !dead[(long long)o * dimz + k];
    const unsigned long long lm = __ballot(live);
    const unsigned m0 = (unsigned)lm, m1 = (unsigned)(lm >> 32);
    const unsigned mh = half ? m1 : m0;
    const int src = mh ? (__ffs(mh) - 1) + 32 * half : lane;        // the group's first live line
    const uint16_t *p = code + (long long)o * os + (live ? k : 0);
    bool uni = true, eq = true;
    unsigned long long h = 0;
    uint16_t *mycol = col + ((long long)o * ng + (have_g ? g : g0)) * UCOL_PITCH;
    for (int s = 0; s < n; s++) {
        const int v = live ? (p[(long long)s * ss] & keep) : 0;
        const int ref = mh ? __shfl(v, src, 64) : 0;
        const unsigned long long ne = __ballot(live && v != ref);
        if ((unsigned)(half ? ne >> 32 : ne)) uni = false;
        if (__shfl(ref, 0, 64) != __shfl(ref, 32, 64)) eq = false;
        h = geom_mix(h ^ (unsigned long long)(ref + 1) ^ ((unsigned long long)s << 20));
        if ((lane & 31) == 0 && have_g) mycol[s] = (uint16_t)ref;
    }
    const bool u0 = __shfl((int)uni, 0, 64), u1 = __shfl((int)uni, 32, 64);
    const bool da = m0 == 0, db = m1 == 0;
    const bool have_b = g0 + 1 < ng;
    bool pair = u0;
    if (have_b) pair = u0 && u1 && (da || db || eq);
    unsigned long long h0 = __shfl(h, 0, 64);
    const unsigned long long h1 = __shfl(h, 32, 64);
    if (have_b && u0 && u1 && da && !db) {
        // an all-dead group holds zeros: it takes the other group's column
        __threadfence();
        __syncthreads();
        uint16_t *a = col + ((long long)o * ng + g0) * UCOL_PITCH;
        const uint16_t *b = a + UCOL_PITCH;
        for (int s = lane; s < n; s += 64) a[s] = b[s];
        h0 = h1;
    }
    if (lane == 0) {
        cflag[(long long)o * ng + g0] = (uint8_t)((u0 ? 1 : 0) | (pair ? 2 : 0));
        hash[(long long)o * ng + g0] = h0;
        if (have_b) { cflag[(long long)o * ng + g0 + 1] = u1 ? 1 : 0; hash[(long long)o * ng + g0 + 1] = h1; }
    }
}

// the distinct columns, in the order the host numbered them
__global__ void __launch_bounds__(256) k_geom_gather(const uint16_t *__restrict__ col, const int *__restrict__ rep, uint16_t *__restrict__ ucol)
{
    const uint16_t *s = col + (long long)rep[blockIdx.x] * UCOL_PITCH;
    uint16_t *d = ucol + (long long)blockIdx.x * UCOL_PITCH;
    for (int t = threadIdx.x; t < UCOL_PITCH; t += 256) d[t] = s[t];
}

// every uniform group's own column against the column its flag word names: the host decided identities from hashes, the device
// confirms them cell by cell (a difference fails the update instead of letting a sweep read another column's codes)
__global__ void __launch_bounds__(64) k_geom_verify(const uint16_t *__restrict__ col, const unsigned *__restrict__ uflag,
                                                     const uint16_t *__restrict__ ucol, int n, unsigned long long *cnt)
{
    const unsigned f = uflag[blockIdx.x];
    if (!(f & 3)) return;
    const uint16_t *a = col + (long long)blockIdx.x * UCOL_PITCH, *b = ucol + (long long)(f >> 2) * UCOL_PITCH;
    bool bad = false;
    for (int s = threadIdx.x; s < n; s += 64) bad |= a[s] != b[s];
    if (__ballot(bad) && threadIdx.x == 0) atomicAdd(&cnt[GC_MISMATCH], 1ull);
}

// order-independent digest of the cell-code table: the sum over cells of a mix of (cell index, code), modulo 2^64
__global__ void __launch_bounds__(256) k_geom_digest(const uint16_t *__restrict__ code, long long ncell, unsigned long long *out)
{
    unsigned long long acc = 0;
    for (long long l = (long long)blockIdx.x * 256 + threadIdx.x; l < ncell; l += (long long)gridDim.x * 256)
        acc += geom_mix(((unsigned long long)l << 16) | code[l]);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

// TimeLayer3D::Clear(grid, NODE_OUT, 0, 0, 0, baseT) (TimeLayer3D.h:974-999) on one layer
template <typename R>
__global__ void __launch_bounds__(256) k_clear_outer(const uint16_t *__restrict__ code, long long n, R baseT, R *d0, R *d1, R *d2, R *d3)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        if (((code[i] >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_OUT) { d0[i] = R(0); d1[i] = R(0); d2[i] = R(0); d3[i] = baseT; }
}

// Grid3D::Prepare2D (Grid3D.cpp:608-668) as host/Shape2D.h ExtrudeShape2D states it: the node of cell (i, j, k) from the record of
// column (i, j) -- the 2D cell type c2, its velocity and temperature, and `bottom` -- and the scalars A = active_dimz and baseT.
// The host function writes some cells several times and the last write wins; as a priority list, first match decides:
//   1. c2 == NODE_OUT                       OUT,   NOSLIP / NOSLIP, v = 0, T = 0     (the whole column; nothing else is written)
//   2. bottom < k < A - 2  (the middle)     c2 == IN:    IN,    NOSLIP / NOSLIP, v = 0,                T = baseT
//                                           c2 == BOUND: BOUND, NOSLIP / FREE,   v = (velx, vely, 0),  T = T2
//                                           c2 == VALVE: VALVE, FREE / FREE when velx == 0 and vely == 0, else NOSLIP / NOSLIP; v, T as BOUND
//   3. 1 <= k <= bottom    (the floor)      BOUND, NOSLIP / FREE, v = 0, T = baseT   (passes A - 2 and the lid where bottom does)
//   4. k == 0                               OUT by type only: what the bound of A - 2 wrote stays when A == 2 (NOSLIP / FREE, T = baseT),
//                                           else NOSLIP / NOSLIP, v = 0, T = 0
//   5. k == A - 2          (the bound)      BOUND, NOSLIP / FREE, v = 0, T = baseT
//   6. k >= A - 1          (the lid)        OUT,   NOSLIP / NOSLIP, v = 0, T = 0
// (host order: memset, 1, 6, 5, 4, 3, 2.)  vz is 0 everywhere.  No arithmetic: 2D floats widen to R exactly.
struct ExNode { int type, bv, bt; float vx, vy, T; };

__device__ __forceinline__ ExNode extrude_node(int k, int c2, float velx, float vely, float T2, int bottom, int A, float baseT)
{
    ExNode n = {FS3D_NODE_OUT, FS3D_BC_NOSLIP, FS3D_BC_NOSLIP, 0.0f, 0.0f, 0.0f};
    if (c2 == FS3D_NODE_OUT) return n;
    if (k > bottom && k < A - 2) {
        n.type = c2;
        if (c2 == FS3D_NODE_IN) { n.T = baseT; return n; }
        const bool rest = c2 == FS3D_NODE_VALVE && velx == 0.0f && vely == 0.0f;
        n.bv = rest ? FS3D_BC_FREE : FS3D_BC_NOSLIP;
        n.bt = (rest || c2 == FS3D_NODE_BOUND) ? FS3D_BC_FREE : FS3D_BC_NOSLIP;
        n.vx = velx; n.vy = vely; n.T = T2;
        return n;
    }
    const bool floor_ = k >= 1 && k <= bottom;
    if (floor_ || k == A - 2) {                         // k == 0 == A - 2: the bound's values under the type of rule 4
        n.type = (floor_ || k != 0) ? FS3D_NODE_BOUND : FS3D_NODE_OUT;
        n.bt = FS3D_BC_FREE; n.T = baseT;
    }
    return n;
}

// Pure store kernel, 19 bytes per cell in fp32 and 35 in fp64.  One thread writes V consecutive k of one column: V == 4 (dimz % 4 == 0,
// the byte arrays aligned to 4 bytes and the value arrays to 16) one dword per byte array and 16-byte stores for the value arrays
// (one per array in fp32, two in fp64), V == 1 cell by cell.
// Lanes run along k, so a wave writes 64 * V consecutive cells; the column record is read once per thread.  Stores are nontemporal:
// the geometry kernels read these arrays next, but only after the whole grid has been written.
template <typename R, int V>
__global__ void __launch_bounds__(256) k_geom_extrude(const float *__restrict__ velx, const float *__restrict__ vely, const float *__restrict__ T2,
                                                       const int *__restrict__ bottom, const uint8_t *__restrict__ cell, long long ncol, int dimz,
                                                       int A, float baseT, uint8_t *__restrict__ type, uint8_t *__restrict__ bc_vel,
                                                       uint8_t *__restrict__ bc_temp, R *__restrict__ vx, R *__restrict__ vy, R *__restrict__ vz,
                                                       R *__restrict__ T)
{
    constexpr int P = 16 / sizeof(R);                  // values per 16-byte store
    typedef R RP __attribute__((ext_vector_type(P)));
    const int nq = dimz / V;                           // V == 4: dimz % 4 == 0
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ncol * nq) return;
    const long long col = t / nq;
    const int k0 = (int)(t - col * nq) * V;
    const int c2 = cell[col], bot = bottom[col];
    const float ux = velx[col], uy = vely[col], t2 = T2[col];
    const long long l = col * dimz + k0;               // < ncol * dimz: the arrays' size
    unsigned wt = 0, wv = 0, wb = 0;
    R ax[V], ay[V], aT[V];
#pragma unroll
    for (int q = 0; q < V; q++) {
        const ExNode n = extrude_node(k0 + q, c2, ux, uy, t2, bot, A, baseT);
        wt |= (unsigned)n.type << (8 * q); wv |= (unsigned)n.bv << (8 * q); wb |= (unsigned)n.bt << (8 * q);
        ax[q] = (R)n.vx; ay[q] = (R)n.vy; aT[q] = (R)n.T;
    }
    if constexpr (V == 4) {
        __builtin_nontemporal_store(wt, (unsigned *)(type + l));
        __builtin_nontemporal_store(wv, (unsigned *)(bc_vel + l));
        __builtin_nontemporal_store(wb, (unsigned *)(bc_temp + l));
#pragma unroll
        for (int h = 0; h < V; h += P) {
            RP x, y, z, w;
#pragma unroll
            for (int q = 0; q < P; q++) { x[q] = ax[h + q]; y[q] = ay[h + q]; z[q] = R(0); w[q] = aT[h + q]; }
            __builtin_nontemporal_store(x, (RP *)(vx + l + h));
            __builtin_nontemporal_store(y, (RP *)(vy + l + h));
            __builtin_nontemporal_store(z, (RP *)(vz + l + h));
            __builtin_nontemporal_store(w, (RP *)(T + l + h));
        }
    } else {
        __builtin_nontemporal_store((uint8_t)wt, type + l);
        __builtin_nontemporal_store((uint8_t)wv, bc_vel + l);
        __builtin_nontemporal_store((uint8_t)wb, bc_temp + l);
        __builtin_nontemporal_store(ax[0], vx + l);
        __builtin_nontemporal_store(ay[0], vy + l);
        __builtin_nontemporal_store(R(0), vz + l);
        __builtin_nontemporal_store(aT[0], T + l);
    }
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------

static inline unsigned geom_grid(long long n, int cap = 4096)
{
    const long long g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// lines / groups of the shared columns of direction d
static inline int geom_n_o(const fs3d_ctx *c, int d) { return d == 0 ? c->dimy : c->dimx; }
static inline int geom_n(const fs3d_ctx *c, int d) { return d == 0 ? c->dimx : c->dimy; }
static inline int geom_ng(const fs3d_ctx *c) { return (c->dimz + 31) / 32; }

// Device time of an update, while fs3d_enable_timing is on: an event before the first launch of every batch and one before the
// synchronisation that ends it (the host's work between two batches is not device time).
static void gev_begin(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    if (!c->timing_period || g.ev_open || g.ev_n + 2 > 16) return;
    for (int k = g.ev_n; k < g.ev_n + 2; k++) if (!g.ev[k] && hipEventCreate(&g.ev[k]) != hipSuccess) return;
    hipEventRecord(g.ev[g.ev_n], c->stream);
    g.ev_open = true;
}
static void gev_end(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    if (!g.ev_open) return;
    hipEventRecord(g.ev[g.ev_n + 1], c->stream);
    g.ev_n += 2; g.ev_open = false;
}
static void gev_collect(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    gev_end(c);
    g.last_dev_ms = 0;
    for (int k = 0; k + 1 < g.ev_n; k += 2) {
        float ms = 0;
        if (hipEventSynchronize(g.ev[k + 1]) == hipSuccess && hipEventElapsedTime(&ms, g.ev[k], g.ev[k + 1]) == hipSuccess) g.last_dev_ms += ms;
    }
    g.ev_n = 0;
}

void fs3d_geom_destroy(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    for (hipEvent_t e : g.ev) if (e) hipEventDestroy(e);
    if (g.stage) hipFree(g.stage);
    for (int d = 0; d < 3; d++) if (g.lst[d]) hipFree(g.lst[d]);
    for (int d = 0; d < 2; d++) {
        if (g.col[d]) hipFree(g.col[d]);
        if (g.cflag[d]) hipFree(g.cflag[d]);
        if (g.hash[d]) hipFree(g.hash[d]);
        if (g.rep[d]) hipFree(g.rep[d]);
    }
    if (g.cnt) hipFree(g.cnt);
    if (g.host) hipHostFree(g.host);
    if (g.ex_host) hipHostFree(g.ex_host);
    if (g.ex_dev) hipFree(g.ex_dev);
}

// the buffers an update keeps: allocated by the first one
static fs3d_status geom_prepare(fs3d_ctx *c, bool need_stage)
{
    fs3d_geom &g = c->geom;
    const long long nl[3] = {(long long)c->dimy * c->dimz, (long long)c->dimx * c->dimz, (long long)c->dimx * c->dimy};
    if (need_stage && !g.stage) GMALLOC(c, &g.stage, (size_t)3 * c->ncell);
    if (g.cnt) return FS3D_OK;
    for (int d = 0; d < 3; d++) GMALLOC(c, &g.lst[d], (size_t)nl[d] * sizeof(int));
    size_t host_bytes = GC_WORDS * sizeof(unsigned long long);
    for (int d = 0; d < 2; d++) {
        if (geom_n(c, d) > UCOL_PITCH) continue;         // as upload_nodes_impl: no shared columns for longer lines
        const size_t nq = (size_t)geom_n_o(c, d) * geom_ng(c);
        GMALLOC(c, &g.col[d], nq * UCOL_PITCH * sizeof(uint16_t));
        GHIP(c, hipMemsetAsync(g.col[d], 0, nq * UCOL_PITCH * sizeof(uint16_t), c->stream));
        GMALLOC(c, &g.cflag[d], nq);
        GMALLOC(c, &g.hash[d], nq * sizeof(unsigned long long));
        GMALLOC(c, &g.rep[d], nq * sizeof(int));
        host_bytes = std::max(host_bytes, nq * (sizeof(unsigned long long) + sizeof(unsigned) + sizeof(int) + 1) + 64);
    }
    GHIP(c, hipHostMalloc((void **)&g.host, host_bytes, hipHostMallocDefault));
    GMALLOC(c, &g.cnt, GC_WORDS * sizeof(unsigned long long));
    return FS3D_OK;
}

// shared columns of direction d from the new code table (dead[d] is current)
static fs3d_status geom_columns(fs3d_ctx *c, int d)
{
    fs3d_geom &g = c->geom;
    const int n_o = geom_n_o(c, d), n = geom_n(c, d), ng = geom_ng(c);
    if (n > UCOL_PITCH) { c->n_ucol[d] = 0; return FS3D_OK; }
    const size_t nq = (size_t)n_o * ng;
    if (c->ucol_cap[d] < (long long)nq) {                // the upload's table holds its own distinct columns only: once, room for any number
        gfree(c, c->ucol[d]); c->ucol[d] = nullptr; c->ucol_cap[d] = 0;
        GMALLOC(c, &c->ucol[d], nq * UCOL_PITCH * sizeof(uint16_t));
        c->ucol_cap[d] = (long long)nq;
    }
    const int keep = (0xF << (4 * d)) | (3 << CODE_TYPE_SHIFT);
    const long long ss = d == 0 ? c->plane : c->dimz, os = d == 0 ? (long long)c->dimz : c->plane;
    gev_begin(c);
    hipLaunchKernelGGL(k_geom_columns, dim3((unsigned)(n_o * ((ng + 1) / 2))), dim3(64), 0, c->stream, c->code, c->dead[d], ng, c->dimz,
                       os, ss, n, keep, g.col[d], g.cflag[d], g.hash[d]);
    GHIP(c, hipGetLastError());
    // identities on the host from the hashes (a few KB), numbered in the order of first appearance as upload_nodes_impl numbers them
    unsigned long long *hh = (unsigned long long *)g.host;
    unsigned *fl = (unsigned *)(hh + nq);
    int *rep = (int *)(fl + nq);
    uint8_t *cf = (uint8_t *)(rep + nq);
    GHIP(c, hipMemcpyAsync(hh, g.hash[d], nq * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    GHIP(c, hipMemcpyAsync(cf, g.cflag[d], nq, hipMemcpyDeviceToHost, c->stream));
    gev_end(c);
    GHIP(c, hipStreamSynchronize(c->stream));
    std::unordered_map<unsigned long long, unsigned> ids;
    unsigned nid = 0;
    for (size_t q = 0; q < nq; q++) {
        fl[q] = 0;
        if (!cf[q]) continue;
        auto it = ids.find(hh[q]);
        if (it == ids.end()) { it = ids.emplace(hh[q], nid).first; rep[nid++] = (int)q; }
        fl[q] = (unsigned)cf[q] | (it->second << 2);
    }
    c->n_ucol[d] = (int)nid;
    gev_begin(c);
    GHIP(c, hipMemcpyAsync(c->uflag[d], fl, nq * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    if (nid) {
        GHIP(c, hipMemcpyAsync(g.rep[d], rep, nid * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_geom_gather, dim3(nid), dim3(256), 0, c->stream, g.col[d], g.rep[d], c->ucol[d]);
        hipLaunchKernelGGL(k_geom_verify, dim3((unsigned)nq), dim3(64), 0, c->stream, g.col[d], c->uflag[d], c->ucol[d], n, g.cnt);
        GHIP(c, hipGetLastError());
    }
    // the pinned block is reused by the next direction: its copies must have left
    gev_end(c);
    GHIP(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

template <typename R>
static fs3d_status update_nodes_impl(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp, int n_seg_out[3])
{
    fs3d_geom &g = c->geom;
    const int dx = c->dimx, dy = c->dimy, dz = c->dimz;
    const long long plane = c->plane, ncell = c->ncell;
    GHIP(c, hipMemsetAsync(g.cnt, 0, GC_WORDS * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_geom_lines_strided, dim3(geom_grid((long long)dy * dz, 1 << 30)), dim3(256), 0, c->stream, type, dy, dz,
                       (long long)dz, plane, dx, g.lst[0], c->dead[0]);
    hipLaunchKernelGGL(k_geom_lines_strided, dim3(geom_grid((long long)dx * dz, 1 << 30)), dim3(256), 0, c->stream, type, dx, dz,
                       plane, (long long)dz, dy, g.lst[1], c->dead[1]);
    hipLaunchKernelGGL(k_geom_lines_z, dim3(geom_grid((long long)dx * dy * 64, 1 << 30)), dim3(256), 0, c->stream, type,
                       (long long)dx * dy, dz, g.lst[2], c->dead[2]);
    hipLaunchKernelGGL(k_geom_codes, dim3(geom_grid(ncell)), dim3(256), 0, c->stream, type, bc_vel, bc_temp, g.lst[0], g.lst[1],
                       g.lst[2], dx, dy, dz, c->code, g.cnt);
    GHIP(c, hipGetLastError());
    unsigned long long *hc = (unsigned long long *)g.host;
    GHIP(c, hipMemcpyAsync(hc, g.cnt, GC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    gev_end(c);
    GHIP(c, hipStreamSynchronize(c->stream));
    if (hc[GC_SHARED])
        return gfail(c, FS3D_ERR_UNSUPPORTED,
                     "fs3d_update_nodes: a cell with a FREE boundary condition closes one segment and opens the next "
                     "on the same line (two rows on one cell; the reference's result there depends on thread timing)");
    const long long nseg[3] = {(long long)hc[0], (long long)hc[1], (long long)hc[2]};
    const long long nbnd = (long long)hc[GC_NBND];
    c->stale_in_cells = (long long)hc[GC_STALE];
    // BOUND / VALVE list: grow-only
    if (nbnd > c->bnd_cap) {
        gfree(c, c->bnd_idx); c->bnd_idx = nullptr;
        for (int v = 0; v < 4; v++) { gfree(c, c->bnd_val[v]); c->bnd_val[v] = nullptr; }
        c->bnd_cap = 0; c->n_bnd = 0;
        const long long cap = std::min<long long>(ncell, nbnd + nbnd / 4 + 1024);      // headroom: the list of a moving wall breathes
        GMALLOC(c, &c->bnd_idx, sizeof(int) * (size_t)cap);
        for (int v = 0; v < 4; v++) GMALLOC(c, &c->bnd_val[v], sizeof(R) * (size_t)cap);
        c->bnd_cap = (int)cap;
    }
    if (nbnd) {
        gev_begin(c);
        hipLaunchKernelGGL((k_geom_bnd_list<R>), dim3(geom_grid((ncell + GEOM_LIST_CHUNKS - 1) / GEOM_LIST_CHUNKS)), dim3(256), 0, c->stream, type, ncell, (const R *)c->node,
                           c->nstride, c->bnd_cap, c->bnd_idx, (R *)c->bnd_val[0], (R *)c->bnd_val[1], (R *)c->bnd_val[2],
                           (R *)c->bnd_val[3], g.cnt);
        GHIP(c, hipGetLastError());
    }
    for (int d = 0; d < 2; d++) { const fs3d_status st = geom_columns(c, d); if (st) return st; }
    gev_begin(c);
    GHIP(c, hipMemcpyAsync(hc, g.cnt, GC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    gev_end(c);
    GHIP(c, hipStreamSynchronize(c->stream));
    if ((long long)hc[GC_LIST] != nbnd)
        return gfail(c, FS3D_ERR_HIP, "fs3d_update_nodes: the BOUND / VALVE list does not hold the counted cells");
    if (hc[GC_MISMATCH])
        return gfail(c, FS3D_ERR_HIP, "fs3d_update_nodes: two different shared code columns have the same hash; tables not usable");
    c->n_bnd = (int)nbnd;
    for (int d = 0; d < 3; d++) { c->nseg[d] = (int)nseg[d]; if (n_seg_out) n_seg_out[d] = (int)nseg[d]; }
    return FS3D_OK;
}

// ---- extrusion of a Shape2D grid ----------------------------------------------------------------------------------------------
struct ExtrudeIn { const uint8_t *cell; const float *velx, *vely, *T; double dz, depth, depth_var, baseT; int A; };

#define EX_BOTTOM_BAD INT_MIN

// active_dimz of Grid3D::LoadFromFile (Grid3D.cpp:503-505), for values that give an int
static bool extrude_active_dimz(double dz, double depth, int *A)
{
    if (!(dz > 0) || !(depth >= 0) || !(depth / dz <= 65536.0)) return false;
    *A = (int)std::ceil(depth / dz) + 1;
    return true;
}

// `bottom` of every column with the expression of ExtrudeShape2D (Grid3D.cpp:632-636), on the host and without contraction: a
// last-bit difference in front of (int) moves a wall by a cell.  A product outside int marks the column EX_BOTTOM_BAD.
static void extrude_bottom_table(int dimx, int dimy, int A, double depth_var, int *out)
{
#pragma clang fp contract(off)
    const int height = std::max(A - 2 - 2, 0);
    for (int i = 0; i < dimx; i++)
        for (int j = 0; j < dimy; j++) {
            const double x = -1 + 2 * (double)i / dimx, y = -1 + 2 * (double)j / dimy;
            const double z = 1.0 - (x * x + y * y) * 0.5;
            const double v = depth_var * z * height;
            out[(size_t)i * dimy + j] = (v > -1e9 && v < 1e9) ? 1 + (int)v : EX_BOTTOM_BAD;
        }
}

extern "C" fs3d_status fs3d_shape2d_bottom(int dimx, int dimy, double dz, double depth, double depth_var, int *bottom_out)
{
    int A = 0;
    if (dimx < 1 || dimy < 1 || !bottom_out || !extrude_active_dimz(dz, depth, &A)) return FS3D_ERR_INVALID;
    extrude_bottom_table(dimx, dimy, A, depth_var, bottom_out);
    return FS3D_OK;
}

static inline size_t ex_off_cell(size_t ncol) { return 12 * ncol; }
static inline size_t ex_off_bottom(size_t ncol) { return 12 * ncol + ((ncol + 3) & ~(size_t)3); }
static inline size_t ex_bytes(size_t ncol) { return ex_off_bottom(ncol) + 4 * ncol; }

// Everything that refuses an extrusion, before anything is launched; leaves the column records in the pinned block.
static fs3d_status extrude_check(fs3d_ctx *c, ExtrudeIn &in, const char *name)
{
    fs3d_geom &g = c->geom;
    if (!extrude_active_dimz(in.dz, in.depth, &in.A) || in.A < 2 || in.A > c->dimz)
        return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": active_dimz = ceil(depth / dz) + 1 must lie in 2 .. dimz");
    const size_t ncol = (size_t)c->dimx * c->dimy;
    GHIP(c, hipSetDevice(c->device));
    if (!g.ex_host) GHIP(c, hipHostMalloc(&g.ex_host, ex_bytes(ncol), hipHostMallocDefault));
    if (!g.ex_dev) {                                      // (a failure leaves the pointer null: the next call allocates again)
        GMALLOC(c, &g.ex_dev, ex_bytes(ncol));
        g.ex_bottom_valid = false; g.ex_dz = -1;
    }
    char *h = (char *)g.ex_host;
    int *bottom = (int *)(h + ex_off_bottom(ncol));
    if (g.ex_dz != in.dz || g.ex_depth != in.depth || g.ex_depth_var != in.depth_var) {      // (a NaN depth_var: recomputed every call)
        extrude_bottom_table(c->dimx, c->dimy, in.A, in.depth_var, bottom);
        g.ex_dz = in.dz; g.ex_depth = in.depth; g.ex_depth_var = in.depth_var; g.ex_bottom_valid = false;
    }
    for (size_t q = 0; q < ncol; q++) {
        const uint8_t t = in.cell[q];
        if (t > FS3D_NODE_VALVE) return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": a cell2d value is not a node type");
        // where ExtrudeShape2D would write outside the column's dimz cells (it reads `bottom` of the columns that are not NODE_OUT)
        if (t != FS3D_NODE_OUT && (bottom[q] < -1 || bottom[q] >= c->dimz))
            return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": depth_var puts the bottom of a column outside the grid");
    }
    memcpy(h, in.velx, 4 * ncol); memcpy(h + 4 * ncol, in.vely, 4 * ncol); memcpy(h + 8 * ncol, in.T, 4 * ncol);
    memcpy(h + ex_off_cell(ncol), in.cell, ncol);
    return FS3D_OK;
}

// the column records to the device and the kernel, on the context's stream; not synchronised
template <typename R>
static fs3d_status extrude_launch(fs3d_ctx *c, const ExtrudeIn &in, uint8_t *type, uint8_t *bc_vel, uint8_t *bc_temp, void *vx, void *vy, void *vz, void *T)
{
    fs3d_geom &g = c->geom;
    const size_t ncol = (size_t)c->dimx * c->dimy;
    const char *d = (const char *)g.ex_dev;
    GHIP(c, hipMemcpyAsync(g.ex_dev, g.ex_host, g.ex_bottom_valid ? ex_off_cell(ncol) + ncol : ex_bytes(ncol), hipMemcpyHostToDevice, c->stream));
    g.ex_bottom_valid = true;
    uintptr_t mis = ((uintptr_t)type | (uintptr_t)bc_vel | (uintptr_t)bc_temp) & 3;
    mis |= ((uintptr_t)vx | (uintptr_t)vy | (uintptr_t)vz | (uintptr_t)T) & 15;
    const bool vec = c->dimz % 4 == 0 && !mis;
    const long long nthr = (long long)ncol * (vec ? c->dimz / 4 : c->dimz);
    auto kern = vec ? k_geom_extrude<R, 4> : k_geom_extrude<R, 1>;
    hipLaunchKernelGGL(kern, dim3(geom_grid(nthr, 1 << 30)), dim3(256), 0, c->stream, (const float *)d, (const float *)(d + 4 * ncol),
                       (const float *)(d + 8 * ncol), (const int *)(d + ex_off_bottom(ncol)), (const uint8_t *)(d + ex_off_cell(ncol)),
                       (long long)ncol, c->dimz, in.A, (float)in.baseT, type, bc_vel, bc_temp, (R *)vx, (R *)vy, (R *)vz, (R *)T);
    GHIP(c, hipGetLastError());
    return FS3D_OK;
}

static bool geom_is_slab(const fs3d_ctx *c) { return c->dimx != c->dimx_global || c->x_offset != 0 || c->comm || c->local || c->nranks > 1; }

// ex != nullptr: the seven arrays come from the extrusion kernel (fs3d_update_nodes_shape2d)
static fs3d_status update_nodes_common(fs3d_ctx *c, bool host_arrays, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                       const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3],
                                       const ExtrudeIn *ex = nullptr)
{
    const char *name = ex ? "fs3d_update_nodes_shape2d" : host_arrays ? "fs3d_update_nodes" : "fs3d_update_nodes_dev";
    if (!c) return FS3D_ERR_INVALID;
    if (ex ? (!ex->cell || !ex->velx || !ex->vely || !ex->T) : (!type || !bc_vel || !bc_temp || !vx || !vy || !vz || !T))
        return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": NULL array");
    if (geom_is_slab(c))
        return gfail(c, FS3D_ERR_UNSUPPORTED, std::string(name) + ": moving geometry is implemented for a single context only, "
                     "not for an x-slab of a larger grid or a member of a multi-GPU group");
    if (!c->uploaded_once)
        return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": the first geometry comes through fs3d_upload_nodes; upload nodes first");
    const auto t0 = std::chrono::steady_clock::now();
    GHIP(c, hipSetDevice(c->device));
    fs3d_status st;
    ExtrudeIn exin;
    if (ex) {                                             // refused here, the context keeps the geometry it has
        exin = *ex;
        st = extrude_check(c, exin, name);
        if (st) return st;
    }
    // rebuilt in place: from here until the end the context has no geometry
    c->have_nodes = false;
    st = geom_prepare(c, host_arrays || ex);
    if (st) return st;
    const void *val[4] = {vx, vy, vz, T};
    c->geom.ev_n = 0; c->geom.ev_open = false;
    gev_begin(c);
    if (ex) {
        // the three byte arrays into the staging buffer, the four value fields straight into the node-value table
        uint8_t *sg = c->geom.stage;
        char *nv[4];
        for (int v = 0; v < 4; v++) { nv[v] = (char *)c->node + (size_t)v * c->nstride * c->esize; val[v] = nv[v]; }
        st = c->prec == FS3D_F32 ? extrude_launch<float>(c, exin, sg, sg + c->ncell, sg + 2 * c->ncell, nv[0], nv[1], nv[2], nv[3])
                                 : extrude_launch<double>(c, exin, sg, sg + c->ncell, sg + 2 * c->ncell, nv[0], nv[1], nv[2], nv[3]);
        if (st) return st;
        type = sg; bc_vel = sg + c->ncell; bc_temp = sg + 2 * c->ncell;
    } else if (host_arrays) {
        const uint8_t *src[3] = {type, bc_vel, bc_temp};
        for (int a = 0; a < 3; a++)
            GHIP(c, hipMemcpyAsync(c->geom.stage + (size_t)a * c->ncell, src[a], (size_t)c->ncell, hipMemcpyHostToDevice, c->stream));
        type = c->geom.stage; bc_vel = type + c->ncell; bc_temp = bc_vel + c->ncell;
    }
    // the four node-value fields are one of the tables: copied straight into place
    for (int v = 0; v < 4; v++) {
        char *dst = (char *)c->node + (size_t)v * c->nstride * c->esize;
        if (dst != (const char *)val[v])
            GHIP(c, hipMemcpyAsync(dst, val[v], (size_t)c->ncell * c->esize, host_arrays ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    }
    st = c->prec == FS3D_F32 ? update_nodes_impl<float>(c, type, bc_vel, bc_temp, n_seg_out)
                             : update_nodes_impl<double>(c, type, bc_vel, bc_temp, n_seg_out);
    hipStreamSynchronize(c->stream);                      // (a failure half way: the caller's arrays are not read after the call returns)
    gev_collect(c);
    if (st == FS3D_OK) { c->have_nodes = true; c->n_create_segments++; }
    c->t_create_segments_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

extern "C" fs3d_status fs3d_update_nodes(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                         const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    return update_nodes_common(c, true, type, bc_vel, bc_temp, vx, vy, vz, T, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_dev(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                             const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    return update_nodes_common(c, false, type, bc_vel, bc_temp, vx, vy, vz, T, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape2d(fs3d_ctx *c, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                                 double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{
    const ExtrudeIn in = {cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT, 0};
    return update_nodes_common(c, false, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, n_seg_out, &in);
}

extern "C" fs3d_status fs3d_extrude_shape2d_dev(fs3d_ctx *c, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                                double dz, double depth, double depth_var, double baseT, uint8_t *type_out,
                                                uint8_t *bc_vel_out, uint8_t *bc_temp_out, void *vx_out, void *vy_out, void *vz_out, void *T_out)
{
    const char *name = "fs3d_extrude_shape2d_dev";
    if (!c) return FS3D_ERR_INVALID;
    if (!cell2d || !velx2d || !vely2d || !T2d || !type_out || !bc_vel_out || !bc_temp_out || !vx_out || !vy_out || !vz_out || !T_out)
        return gfail(c, FS3D_ERR_INVALID, std::string(name) + ": NULL array");
    if (geom_is_slab(c))
        return gfail(c, FS3D_ERR_UNSUPPORTED, std::string(name) + ": the extrusion is implemented for a single context only, "
                     "not for an x-slab of a larger grid or a member of a multi-GPU group");
    ExtrudeIn in = {cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT, 0};
    fs3d_status st = extrude_check(c, in, name);
    if (st) return st;
    st = c->prec == FS3D_F32 ? extrude_launch<float>(c, in, type_out, bc_vel_out, bc_temp_out, vx_out, vy_out, vz_out, T_out)
                             : extrude_launch<double>(c, in, type_out, bc_vel_out, bc_temp_out, vx_out, vy_out, vz_out, T_out);
    if (st) return st;
    GHIP(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_last_update_device_ms(fs3d_ctx *c, float *ms_out)
{
    if (!c || !ms_out) return FS3D_ERR_INVALID;
    *ms_out = c->geom.last_dev_ms;
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_clear_outer_cells(fs3d_ctx *c, int layer, double baseT)
{
    if (!c) return FS3D_ERR_INVALID;
    if (layer < 0 || layer > 3) return gfail(c, FS3D_ERR_INVALID, "fs3d_clear_outer_cells: bad layer id");
    if (!c->have_nodes) return gfail(c, FS3D_ERR_INVALID, "fs3d_clear_outer_cells: upload nodes first");
    GHIP(c, hipSetDevice(c->device));
    char *f[4];
    for (int v = 0; v < 4; v++) f[v] = (char *)c->lay[c->slot[layer]] + ((size_t)v * c->fstride + c->plane) * c->esize;
    if (c->prec == FS3D_F32)
        hipLaunchKernelGGL((k_clear_outer<float>), dim3(geom_grid(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell, (float)baseT,
                           (float *)f[0], (float *)f[1], (float *)f[2], (float *)f[3]);
    else
        hipLaunchKernelGGL((k_clear_outer<double>), dim3(geom_grid(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell, baseT,
                           (double *)f[0], (double *)f[1], (double *)f[2], (double *)f[3]);
    GHIP(c, hipGetLastError());
    GHIP(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_geometry_info(fs3d_ctx *c, long long info[FS3D_N_GEOM_INFO])
{
    if (!c || !info) return FS3D_ERR_INVALID;
    if (!c->have_nodes) return gfail(c, FS3D_ERR_INVALID, "fs3d_geometry_info: upload nodes first");
    GHIP(c, hipSetDevice(c->device));
    for (int k = 0; k < FS3D_N_GEOM_INFO; k++) info[k] = 0;
    for (int d = 0; d < 3; d++) info[d] = c->nseg[d];
    info[3] = c->n_bnd;
    info[4] = c->stale_in_cells;
    const long long nl[3] = {(long long)c->dimy * c->dimz, (long long)c->dimx * c->dimz, (long long)c->dimx * c->dimy};
    std::vector<uint8_t> hb;
    for (int d = 0; d < 3; d++) {
        hb.resize((size_t)nl[d]);
        GHIP(c, hipMemcpyAsync(hb.data(), c->dead[d], (size_t)nl[d], hipMemcpyDeviceToHost, c->stream));
        GHIP(c, hipStreamSynchronize(c->stream));
        for (uint8_t b : hb) info[5 + d] += b != 0;
    }
    for (int d = 0; d < 2; d++) {
        if (!c->uflag[d]) continue;
        std::vector<unsigned> fl((size_t)geom_n_o(c, d) * geom_ng(c));
        GHIP(c, hipMemcpyAsync(fl.data(), c->uflag[d], fl.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        GHIP(c, hipStreamSynchronize(c->stream));
        for (unsigned f : fl) info[8 + d] += f & 1;
        info[10 + d] = c->n_ucol[d];
    }
    // the digest comes from the table the sweeps read; its device word is borrowed from the EvalDivError partials (rewritten by every evaluation)
    unsigned long long *dw = (unsigned long long *)c->red_buf, hw = 0;
    GHIP(c, hipMemsetAsync(dw, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_geom_digest, dim3(geom_grid(c->ncell, 1024)), dim3(256), 0, c->stream, c->code, c->ncell, dw);
    GHIP(c, hipGetLastError());
    GHIP(c, hipMemcpyAsync(&hw, dw, sizeof hw, hipMemcpyDeviceToHost, c->stream));
    GHIP(c, hipStreamSynchronize(c->stream));
    info[12] = (long long)hw;
    info[13] = c->geom_allocs;
    return FS3D_OK;
}
