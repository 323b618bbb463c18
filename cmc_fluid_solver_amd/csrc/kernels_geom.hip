// Moving geometry: the tables the sweeps read, rebuilt on the device between time steps
// (fs3d_update_nodes / fs3d_update_nodes_dev), Solver3D::ClearOutterCells (fs3d_clear_outer_cells) and the
// table summary fs3d_geometry_info.  build_geom_tables (fs3d_tables.h, host only; fs3d_upload_nodes writes what it
// returns) stays the first upload and the definition of every table; the kernels here end with the same tables.
// Also the extrusion of a Shape2D grid into the node arrays on the device (k_geom_extrude; fs3d_extrude_shape2d_dev,
// fs3d_update_nodes_shape2d): a moving Shape2D geometry then ships its 2D grid per step, not the 3D node arrays.
// And the voxelisation of a Shape3D mesh (k_geom_raster_mesh, the flood fill k_geom_fill_z / k_geom_fill_strided, k_geom_mesh_nodes;
// fs3d_voxelize_shape3d_dev, fs3d_flood_fill_dev, fs3d_update_nodes_shape3d): a moving mesh ships its vertices per step.
// On an x-slab (fs3d_update_nodes_slab, fs3d_update_nodes_shape2d_slab) every rank is given the global
// input and rebuilds the tables of its own planes, without communication: the X lines come from the global byte arrays
// (k_geom_lines_x_slab, k_geom_codes<true>, k_geom_extrude<.., true>), everything else runs on the slab's planes.  A mesh on an x-slab
// (fs3d_update_nodes_shape3d_slab, fs3d_update_nodes_shape3d_vel_slab) is voxelised and flood-filled over
// the GLOBAL grid by every rank, in the staging buffer that holds the global byte arrays anyway: the fill is global.
// And the fresh cells (k_fresh_classify, k_fresh_round; fs3d_fill_fresh_cells*): a cell that an update
// turned NODE_IN takes the mean of its fluid neighbours, from the previous node types the caller gives or FS3D_OPT_FRESH_CELLS keeps.
// On the slabs of a group (FS3D_OPT_FRESH_CELLS_SLABS) that fill is the one place here where ranks talk: a plane of fields and of
// round tags per neighbour and round, and the counts summed over the ranks (fresh_fill_impl).
// Every fs3d_update_nodes* entry is one statement above update_run, the one body of an update: a source (node arrays, a Shape2D
// grid, a mesh) gives its NULL test, its check and its producer, and a whole-grid context is the slab x_offset = 0, dimx_global = dimx.
//
// Row kinds without the serial walk of line_kinds (fs3d_tables.h): that walk opens a run at `pos` when cell pos + 1 is
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
#include <cstring>
#include <string>
#include <unordered_map>

#include "fs3d_common.h"
#include "fs3d_comm.h"
#include "fs3d_voxel.h"

// counter words of one update (device, read back once)
enum { GC_NSEG = 0 /* 0..2 */, GC_NBND = 3, GC_STALE = 4, GC_SHARED = 5, GC_LIST = 6, GC_MISMATCH = 7, GC_WORDS = 8 };

// ---------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------

__device__ __forceinline__ bool geom_interior(int s, int ty, int lst) { return s >= 1 && ty == FS3D_NODE_IN && s < lst; }

// X and Y lines: cells `ss` apart, neighbouring lines along k contiguous -- one thread per line, lanes along k read coalesced.
// lst[line] = last index whose type is not NODE_IN (-1: none); dead[line] = 1 when the line has no NODE_IN cell (every cell on a
// segment lies on a line with a NODE_IN cell, so this is geom_dead_lines' "no segment cell and no NODE_IN cell").
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

// X lines of an x-slab -- the planes [x0, x0 + nx) of a line of n = dimx_global cells, `type` the GLOBAL array: one thread per line as
// above (o = j, os = dimz, ss = plane).  The kinds of a line come from the whole line, so lst is the global one; a second walk,
// with lst known, counts what only the whole line tells: its START cells (nseg[0] counts the global segments, GeomTables::nseg)
// and its shared cells that carry a FREE condition, on whichever slab they lie.  dead[line] is LOCAL, as geom_dead_lines defines
// it: 1 when no cell of the slab's piece is NODE_IN or on a segment -- a piece that holds only the line's END cell is live, so
// "no NODE_IN cell" does not do here.  The second walk re-reads what the first one left in the caches.
__global__ void __launch_bounds__(256) k_geom_lines_x_slab(const uint8_t *__restrict__ type, const uint8_t *__restrict__ bc_vel,
                                                            const uint8_t *__restrict__ bc_temp, long long nlines, long long ss, int n,
                                                            int x0, int nx, int *__restrict__ lst, uint8_t *__restrict__ dead,
                                                            unsigned long long *cnt)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned starts = 0, shared = 0;
    if (t < nlines) {
        const uint8_t *p = type + t;
        int last = -1;
        for (int s = 0; s < n; s++)
            if (p[(long long)s * ss] != FS3D_NODE_IN) last = s;
        bool inm = false, in0 = false, live = false;      // INTERIOR(s - 1), INTERIOR(s): cell 0 never is
        int t0 = p[0];
        for (int s = 0; s < n; s++) {
            const int tp = s + 1 < n ? p[(long long)(s + 1) * ss] : 0;
            const bool inp = s + 1 < n && geom_interior(s + 1, tp, last);
            if (!in0 && inp) {
                starts++;
                const long long id = t + (long long)s * ss;
                if (inm && (bc_vel[id] == FS3D_BC_FREE || bc_temp[id] == FS3D_BC_FREE)) shared++;
            }
            if (s >= x0 && s < x0 + nx) live |= t0 == FS3D_NODE_IN || inp || inm;      // (INTERIOR cells are NODE_IN)
            inm = in0; in0 = inp; t0 = tp;
        }
        lst[t] = last;
        dead[t] = live ? 0 : 1;
    }
    for (int off = 32; off > 0; off >>= 1) { starts += __shfl_down(starts, off, 64); shared += __shfl_down(shared, off, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (starts) atomicAdd(&cnt[GC_NSEG], (unsigned long long)starts);
        if (shared) atomicAdd(&cnt[GC_SHARED], (unsigned long long)shared);
    }
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
// SLAB: the dimx planes from x0 of a grid of gx planes; `type` addresses the slab's first cell INSIDE the global array (the planes
// x0 - 1 and x0 + dimx are read where they exist) and lstx is the global line's.  The X row code takes the global index; the START
// cells and the shared cells of X are those of k_geom_lines_x_slab, which sees the whole line, and are not counted here.
template <bool SLAB>
__global__ void __launch_bounds__(256) k_geom_codes(const uint8_t *__restrict__ type, const uint8_t *__restrict__ bc_vel,
                                                     const uint8_t *__restrict__ bc_temp, const int *__restrict__ lstx,
                                                     const int *__restrict__ lsty, const int *__restrict__ lstz, int dimx, int dimy,
                                                     int dimz, int x0, int gx, uint16_t *__restrict__ code, unsigned long long *cnt)
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
        const int sx = SLAB ? x0 + i : i, nx = SLAB ? gx : dimx;
        const int rx = geom_row_code(sx, nx, t0, sx >= 1 ? type[l - plane] : 0, sx + 1 < nx ? type[l + plane] : 0,
                                     lstx[rem], bits, &sh[0]);
        const int ry = geom_row_code(j, dimy, t0, j >= 1 ? type[l - dimz] : 0, j + 1 < dimy ? type[l + dimz] : 0,
                                     lsty[(long long)i * dimz + k], bits, &sh[1]);
        const int rz = geom_row_code(k, dimz, t0, k >= 1 ? type[l - 1] : 0, k + 1 < dimz ? type[l + 1] : 0,
                                     lstz[(long long)i * dimy + j], bits, &sh[2]);
        code[l] = (uint16_t)(rx | (ry << 4) | (rz << 8) | ((t0 & 3) << CODE_TYPE_SHIFT));
        if constexpr (!SLAB) acc[0] += (rx & 3) == ROW_START;
        else sh[0] = false;
        acc[1] += (ry & 3) == ROW_START; acc[2] += (rz & 3) == ROW_START;
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

// Shared code columns of direction d (X: o = j, cells along i; Y: o = i, cells along j), as geom_shared_columns defines them: one
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

// Store tail of the two node-writing kernels: the V consecutive cells from l.  wt / wv / wb hold type, bc_vel and bc_temp of cell q
// in byte q (TYPE false: the type array is not written); vz is 0.  V == 4 (l % 4 == 0, the byte arrays aligned to 4 bytes and the
// value arrays to 16): one dword per byte array and 16-byte stores for the value arrays (one per array in fp32, two in fp64);
// V == 1: cell by cell.  az: vz of the V cells where a kernel has one (else vz is 0).  Stores are nontemporal: the geometry kernels
// read these arrays next, but only after the whole grid has been written.
template <int V, bool TYPE>
__device__ __forceinline__ void store_node_bytes(long long l, unsigned wt, unsigned wv, unsigned wb, uint8_t *__restrict__ type,
                                                 uint8_t *__restrict__ bc_vel, uint8_t *__restrict__ bc_temp)
{
    if constexpr (V == 4) {
        if constexpr (TYPE) __builtin_nontemporal_store(wt, (unsigned *)(type + l));
        __builtin_nontemporal_store(wv, (unsigned *)(bc_vel + l));
        __builtin_nontemporal_store(wb, (unsigned *)(bc_temp + l));
    } else {
        if constexpr (TYPE) __builtin_nontemporal_store((uint8_t)wt, type + l);
        __builtin_nontemporal_store((uint8_t)wv, bc_vel + l);
        __builtin_nontemporal_store((uint8_t)wb, bc_temp + l);
    }
}

template <typename R, int V>
__device__ __forceinline__ void store_node_values(long long l, const R (&ax)[V], const R (&ay)[V], const R (&aT)[V], R *__restrict__ vx,
                                                  R *__restrict__ vy, R *__restrict__ vz, R *__restrict__ T, const R *az = nullptr)
{
    constexpr int P = 16 / sizeof(R);                  // values per 16-byte store
    typedef R RP __attribute__((ext_vector_type(P)));
    if constexpr (V == 4) {
#pragma unroll
        for (int h = 0; h < V; h += P) {
            RP x, y, z, w;
#pragma unroll
            for (int q = 0; q < P; q++) { x[q] = ax[h + q]; y[q] = ay[h + q]; z[q] = az ? az[h + q] : R(0); w[q] = aT[h + q]; }
            __builtin_nontemporal_store(x, (RP *)(vx + l + h));
            __builtin_nontemporal_store(y, (RP *)(vy + l + h));
            __builtin_nontemporal_store(z, (RP *)(vz + l + h));
            __builtin_nontemporal_store(w, (RP *)(T + l + h));
        }
    } else {
        __builtin_nontemporal_store(ax[0], vx + l);
        __builtin_nontemporal_store(ay[0], vy + l);
        __builtin_nontemporal_store(az ? az[0] : R(0), vz + l);
        __builtin_nontemporal_store(aT[0], T + l);
    }
}

template <typename R, int V, bool TYPE>
__device__ __forceinline__ void store_nodes(long long l, unsigned wt, unsigned wv, unsigned wb, const R (&ax)[V], const R (&ay)[V],
                                            const R (&aT)[V], uint8_t *__restrict__ type, uint8_t *__restrict__ bc_vel,
                                            uint8_t *__restrict__ bc_temp, R *__restrict__ vx, R *__restrict__ vy, R *__restrict__ vz,
                                            R *__restrict__ T, const R *az = nullptr)
{
    store_node_bytes<V, TYPE>(l, wt, wv, wb, type, bc_vel, bc_temp);
    store_node_values<R, V>(l, ax, ay, aT, vx, vy, vz, T, az);
}

// Pure store kernel, 19 bytes per cell in fp32 and 35 in fp64.  One thread writes V consecutive k of one column (store_nodes;
// V == 4 where dimz % 4 == 0 and the arrays are aligned).
// Lanes run along k, so a wave writes 64 * V consecutive cells; the column record is read once per thread.
// SLAB, the extrusion on an x-slab: `ncol` counts the columns of the GLOBAL grid and the three byte arrays are global (the X lines of
// the slab's tables are read from them), the four value arrays hold the slab's columns [col0, col0 + ncol_own) only -- a thread of
// another slab's column stores its 3 bytes per cell and no values.  Without it all seven arrays cover the ncol columns (col0 and
// ncol_own are not read).  The same node per cell and the same two store shapes.
template <typename R, int V, bool SLAB>
__global__ void __launch_bounds__(256) k_geom_extrude(const float *__restrict__ velx, const float *__restrict__ vely, const float *__restrict__ T2,
                                                       const int *__restrict__ bottom, const uint8_t *__restrict__ cell, long long ncol,
                                                       long long col0, long long ncol_own, int dimz, int A, float baseT,
                                                       uint8_t *__restrict__ type, uint8_t *__restrict__ bc_vel, uint8_t *__restrict__ bc_temp,
                                                       R *__restrict__ vx, R *__restrict__ vy, R *__restrict__ vz, R *__restrict__ T)
{
    const int nq = dimz / V;                           // V == 4: dimz % 4 == 0
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ncol * nq) return;
    const long long col = t / nq;
    const int k0 = (int)(t - col * nq) * V;
    const int c2 = cell[col], bot = bottom[col];
    const float ux = velx[col], uy = vely[col], t2 = T2[col];
    unsigned wt = 0, wv = 0, wb = 0;
    R ax[V], ay[V], aT[V];
#pragma unroll
    for (int q = 0; q < V; q++) {
        const ExNode n = extrude_node(k0 + q, c2, ux, uy, t2, bot, A, baseT);
        wt |= (unsigned)n.type << (8 * q); wv |= (unsigned)n.bv << (8 * q); wb |= (unsigned)n.bt << (8 * q);
        ax[q] = (R)n.vx; ay[q] = (R)n.vy; aT[q] = (R)n.T;
    }
    // col * dimz + k0 < ncol * dimz: the byte arrays' size
    if constexpr (!SLAB) store_nodes<R, V, true>(col * dimz + k0, wt, wv, wb, ax, ay, aT, type, bc_vel, bc_temp, vx, vy, vz, T);
    else {
        store_node_bytes<V, true>(col * dimz + k0, wt, wv, wb, type, bc_vel, bc_temp);
        if (col >= col0 && col < col0 + ncol_own)      // (col - col0) * dimz + k0 < ncol_own * dimz: the value arrays'
            store_node_values<R, V>((col - col0) * dimz + k0, ax, ay, aT, vx, vy, vz, T);
    }
}

// ---- Shape3D meshes: Grid3D::Build (Grid3D.cpp:859-903) on the device ------------------------------------------------------------
// k_geom_raster_mesh restates RasterPolygon + ProjectPointOnPolygon + the three RasterLines of every triangle as host/Shape3D.h and
// its twin cmc_fluid_solver_amd/shape3d.py (_raster_polygon, _raster_line) state them: every fp32 operation is the twin's, in the
// twin's order, rounded after each one (this file is compiled without contraction and with IEEE divide and sqrt).
// The type array is preset to NODE_IN and the ONLY write is NODE_BOUND: the result is the union of the cells every triangle
// touches, so the order of triangles and of cells is free -- that is what makes the rasteriser parallel.  One wave per triangle:
// the scan point p += dp accumulates rounding and is advanced serially by the whole wave, the cells of one scan line
// (i from (int)p.x to last_i) are spread across the lanes; lanes 0..2 then walk one edge line each.
// Guards are the twin's, not the undefined behaviour of the C++ host: a projection whose quotient is not finite or exceeds 2e9 in
// magnitude writes nothing, writes outside the grid are dropped, a degenerate triangle (len not > 0, or the three vertices equal
// within COMP_EPS) draws its edge lines only.  Every loop is bounded: where the twin raises (a scan line of more than
// 4 (dimx + dimy + dimz) + 16 cells, or one that runs away from its end cell) and where it would spin (a scan point that
// p.y += dp.y no longer moves) the wave stops its triangle and sets the flag word; the host refuses the mesh.
#define MESH_COMP_EPS 1e-8
#define MESH_FLAG_SCANLINE 1u
#define MESH_FLAG_STALLED 2u

struct MV2 { float x, y; };

// (int) of the twin for every value it can meet; defined for any float
__device__ __forceinline__ int mesh_int(float v) { return (int)fminf(fmaxf(v, -2.0e9f), 2.0e9f); }

__device__ __forceinline__ bool mesh_close(float a, float b) { return fabs((double)(a - b)) < MESH_COMP_EPS; }

// GetIntersectHorizon (Grid3D.cpp:676-685), the x of the result
__device__ __forceinline__ float mesh_horizon_x(MV2 p1, MV2 p2, MV2 p)
{
    if (mesh_close(p1.y, p2.y)) return p.x;
    return p1.x + ((p2.x - p1.x) * (p.y - p1.y)) / (p2.y - p1.y);
}

__device__ __forceinline__ void mesh_set(uint8_t *type, int i, int j, int k, int dimx, int dimy, int dimz)
{
    if (i >= 0 && j >= 0 && k >= 0 && i < dimx && j < dimy && k < dimz) type[((long long)i * dimy + j) * dimz + k] = FS3D_NODE_BOUND;
}

// the plane of one triangle, seen along its dominant axis: the normal's components on the two scan axes and the dominant one,
// the sizes and strides of the three axes in that order
struct MeshPlane { float na, nb, nd, d; int lima, limb, limd; long long sa, sb, sd; };

// ProjectPointOnPolygon (Grid3D.cpp:688-707): cell (i, j) of the scan plane back onto the polygon's plane
__device__ __forceinline__ void mesh_project(uint8_t *type, const MeshPlane &pl, int i, int j, float ty)
{
    const float kf = (-pl.d - ((float)i * pl.na + ty * pl.nb)) / pl.nd;
    if (!(fabsf(kf) <= 2.0e9f)) return;                      // not finite, or no int
    const int k = (int)kf;
    if (k >= 0 && k < pl.limd && i >= 0 && i < pl.lima && j >= 0 && j < pl.limb) type[i * pl.sa + j * pl.sb + k * pl.sd] = FS3D_NODE_BOUND;
}

// one half of RasterPolygon's scan (the twin's _scan_half); false: the triangle is given up and the flag word set
__device__ __forceinline__ bool mesh_scan_half(uint8_t *type, const MeshPlane &pl, MV2 &p, float yend, MV2 dp, int steps, MV2 e1, MV2 e2,
                                               int di, long long bound, int lane, unsigned *flag)
{
    // a scan point that moves gains at least 2/3 of dp.y per line (round to nearest), and steps * dp.y is the half's height
    const int max_lines = 2 * steps + 16;
    int lines = 0;
    while (p.y < yend) {
        const int j = mesh_int(p.y), last_i = mesh_int(mesh_horizon_x(e1, e2, p)), i0 = mesh_int(p.x);
        const long long cnt = ((long long)last_i - i0) * di + 1;            // cells i0, i0 + di, .., last_i
        if (cnt < 0 || cnt > bound) { if (lane == 0) atomicOr(flag, MESH_FLAG_SCANLINE); return false; }
        for (long long q = lane; q < cnt; q += 64) mesh_project(type, pl, i0 + (int)q * di, j, p.y);
        const float ny = p.y + dp.y;
        if (!(ny > p.y) || ++lines > max_lines) { if (lane == 0) atomicOr(flag, MESH_FLAG_STALLED); return false; }
        p.x = p.x + dp.x; p.y = ny;
    }
    return true;
}

__global__ void __launch_bounds__(64) k_geom_raster_mesh(const float *__restrict__ vx, const float *__restrict__ vy, const float *__restrict__ vz,
                                                          const int *__restrict__ tri, int dimx, int dimy, int dimz, uint8_t *type, unsigned *flag)
{
    const int lane = threadIdx.x;
    const int i1 = tri[3 * blockIdx.x], i2 = tri[3 * blockIdx.x + 1], i3 = tri[3 * blockIdx.x + 2];
    const float p1x = vx[i1], p1y = vy[i1], p1z = vz[i1], p2x = vx[i2], p2y = vy[i2], p2z = vz[i2], p3x = vx[i3], p3y = vy[i3], p3z = vz[i3];
    // RasterPolygon (Grid3D.cpp:709-789), wave-uniform up to the cells of a scan line
    const bool same = mesh_close(p1x, p2x) && mesh_close(p1y, p2y) && mesh_close(p1z, p2z) && mesh_close(p1x, p3x) && mesh_close(p1y, p3y) && mesh_close(p1z, p3z);
    const float ax = p2x - p1x, ay = p2y - p1y, az = p2z - p1z, bx = p3x - p1x, by = p3y - p1y, bz = p3z - p1z;
    float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!same && len > 0) {
        const float t = 1.0f / len;
        nx = nx * t; ny = ny * t; nz = nz * t;
        const float d = -((p1x * nx + p1y * ny) + p1z * nz);
        MeshPlane pl;
        const float fx = fabsf(nx), fy = fabsf(ny), fz = fabsf(nz), maxv = fmaxf(fx, fmaxf(fy, fz));
        int dir = 0;
        if (mesh_close(maxv, fy)) dir = 1;
        if (mesh_close(maxv, fz)) dir = 2;
        const long long plane = (long long)dimy * dimz;
        MV2 pp1, pp2, pp3, mid;
        if (dir == 0) { pp1 = {p1y, p1z}; pp2 = {p2y, p2z}; pp3 = {p3y, p3z}; pl = {ny, nz, nx, d, dimy, dimz, dimx, dimz, 1, plane}; }
        else if (dir == 1) { pp1 = {p1x, p1z}; pp2 = {p2x, p2z}; pp3 = {p3x, p3z}; pl = {nx, nz, ny, d, dimx, dimz, dimy, plane, 1, dimz}; }
        else { pp1 = {p1x, p1y}; pp2 = {p2x, p2y}; pp3 = {p3x, p3y}; pl = {nx, ny, nz, d, dimx, dimy, dimz, plane, dimz, 1}; }
        if (pp3.y < pp2.y) { mid = pp3; pp3 = pp2; pp2 = mid; }
        if (pp1.y > pp2.y) { mid = pp1; pp1 = pp2; pp2 = mid; }
        if (pp3.y < pp2.y) { mid = pp3; pp3 = pp2; pp2 = mid; }
        mid.x = mesh_horizon_x(pp1, pp3, pp2); mid.y = pp2.y;
        const MV2 dir1 = {mid.x - pp1.x, mid.y - pp1.y}, dir2 = {pp3.x - mid.x, pp3.y - mid.y};
        const int steps1 = mesh_int(fmaxf(fabsf(dir1.x), fabsf(dir1.y))) + 1, steps2 = mesh_int(fmaxf(fabsf(dir2.x), fabsf(dir2.y))) + 1;
        const MV2 dp1 = {dir1.x / (float)steps1, dir1.y / (float)steps1}, dp2 = {dir2.x / (float)steps2, dir2.y / (float)steps2};
        const int di = mid.x < pp2.x ? 1 : -1;
        const long long bound = 4LL * ((long long)dimx + dimy + dimz) + 16;
        MV2 p = pp1;
        if (!mesh_scan_half(type, pl, p, mid.y, dp1, steps1, pp1, pp2, di, bound, lane, flag)) return;
        if (!mesh_scan_half(type, pl, p, pp3.y, dp2, steps2, pp2, pp3, di, bound, lane, flag)) return;
    }
    // RasterLine (Grid3D.cpp:791-811) of (p1, p2), (p1, p3), (p3, p2): one lane each
    if (lane < 3) {
        const float sx = lane == 2 ? p3x : p1x, sy = lane == 2 ? p3y : p1y, sz = lane == 2 ? p3z : p1z;
        const float ex = lane == 1 ? p3x : p2x, ey = lane == 1 ? p3y : p2y, ez = lane == 1 ? p3z : p2z;
        const float dx = ex - sx, dy = ey - sy, dz = ez - sz;
        const int steps = mesh_int(fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)))) + 1;        // coordinates are at most 65536: 131073 steps at most
        const float qx = dx / (float)steps, qy = dy / (float)steps, qz = dz / (float)steps;
        float x = sx, y = sy, z = sz;
        for (int s = 0; s <= steps; s++) {
            mesh_set(type, mesh_int(x), mesh_int(y), mesh_int(z), dimx, dimy, dimz);
            x = x + qx; y = y + qy; z = z + qz;
        }
    }
}

// ---- conservative voxelisation (FS3D_OPT_MESH_VOXELS = 1) -------------------------------------------------------------------------
// k_geom_voxel_mesh: NODE_BOUND iff a triangle overlaps the cell's closed unit box.  The rule -- set-up, column, cell test -- is
// fs3d_voxel.h, which the host loader (host/Shape3D.h) runs as well: one C++ text, specified by Shape3D._voxel_setup /
// _voxel_triangle of cmc_fluid_solver_amd/shape3d.py (where the slack and its derivation stand).  What is here belongs to the device:
// the vertex loads, the strides, the loops, the stores.  One wave per triangle; the set-up (clipped bounding box, local
// vertices, normal, the nine edge functions, the plane's two constants) is wave-uniform.  The three axes are renamed (a, b, d)
// with d the depth axis -- the normal's dominant axis, so the columns of the (a, b) projection that pass its three edge functions
// number about the triangle's area; the lanes stride over the columns of the clipped box.  A column takes its depth range from the
// plane (one cell of margin each way: the range only bounds the loop, every cell in it runs all remaining tests as the twin's do);
// a degenerate triangle has no plane and walks the box's depth, along its smallest extent.  The only write is a byte store of
// NODE_BOUND into an array preset to NODE_IN: idempotent, so order is free and no atomics are needed.  Every index lies inside
// the clipped box; there is no scan line, no guard and no flag word.
// The per-cell loop is neither vectorised nor interleaved: the cell test is one boolean and the store a plain predicated one, which
// the loop vectoriser would take four cells of a column at a time -- four times the live float64 values (242 VGPRs with THIN, two
// waves per SIMD) for columns that are a few cells deep.
// THIN (FS3D_OPT_MESH_SHELL = 1): of the cells that pass, a non-degenerate triangle sets those whose centre cross it meets -- the
// filter of shape3d.py (SHELL_MODES), on the values the conservative test has just computed; its half-widths are wave-uniform.
// OWNER (the entries with wall velocities): every store of NODE_BOUND comes with an integer atomicMin of the triangle's index into
// the cell's word of `owner`, preset to all ones -- the owner of a wall cell is the smallest index of the triangles that set it
// (shape3d.py), a minimum over a set: nothing depends on the order of arrival, and no float atomics take part.  `owner` holds the
// planes [own_x0, own_x0 + own_nx) of the grid only (an x-slab: dimx is the GLOBAL grid's and the bytes go to the global type array,
// the owners of the slab's own cells to its own array; a single context: 0 and dimx): the atomicMin is issued inside that window,
// at the index relative to its first plane.
template <bool OWNER, bool THIN>
__global__ void __launch_bounds__(64) k_geom_voxel_mesh(const float *__restrict__ vx, const float *__restrict__ vy, const float *__restrict__ vz,
                                                         const int *__restrict__ tri, int dimx, int dimy, int dimz, uint8_t *type, unsigned *owner,
                                                         int own_x0, int own_nx)
{
    const int lane = threadIdx.x;
    const int iv[3] = {tri[3 * blockIdx.x], tri[3 * blockIdx.x + 1], tri[3 * blockIdx.x + 2]};
    float p[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) { p[i][0] = vx[iv[i]]; p[i][1] = vy[iv[i]]; p[i][2] = vz[iv[i]]; }
    VoxelSetup s;
    if (!voxel_setup<THIN>(p, dimx, dimy, dimz, s)) return;                                        // (wave-uniform)
    const long long plane = (long long)dimy * dimz;
    const long long sa = voxel_sel(s.a, plane, (long long)dimz, 1LL), sb = voxel_sel(s.b, plane, (long long)dimz, 1LL),
                    sd = voxel_sel(s.d, plane, (long long)dimz, 1LL);
    uint8_t *const base = type + (((long long)s.o[0] * dimy + s.o[1]) * dimz + s.o[2]);
    const int cnt_b = s.cnt[1], ncol = s.cnt[0] * cnt_b;   // at most 8194^2
#pragma unroll 1
    for (int col = lane; col < ncol; col += 64) {
        const int ia = col / cnt_b, ib = col - ia * cnt_b;
        VoxelColumn c;
        if (!voxel_column<THIN>(s, ia, ib, c)) continue;
        uint8_t *const colp = base + ia * sa + ib * sb;
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
        for (int k = c.k0; k <= c.k1; k++) {
            if (!voxel_cell<THIN>(s, c, k)) continue;
            colp[k * sd] = FS3D_NODE_BOUND;
            if constexpr (OWNER) {
                const int ix = s.o[0] + (s.a == 0 ? ia : (s.b == 0 ? ib : k)) - own_x0;                    // the cell's plane, in the window
                if (ix >= 0 && ix < own_nx) atomicMin(owner + (((colp - type) + k * sd) - own_x0 * plane), (unsigned)blockIdx.x);      // < own_nx * plane
            }
        }
    }
}

// FloodFill (Grid3D.cpp:813-857): NODE_OUT spreads from cell (0,0,0) through NODE_IN cells over the 6-neighbourhood.  The result is
// the connected component of that cell, so it does not depend on the order: here as directional passes over the byte array, each
// of which carries NODE_OUT along every line of its direction as far as the line's NODE_IN cells reach (both ways), repeated by
// the host until a whole round of three passes changes nothing.  *cnt counts the cells a pass turns.
__device__ __forceinline__ void fill_block_count(unsigned n, unsigned *cnt)
{
    __shared__ unsigned s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    if (n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(cnt, s_n);
}

// X and Y lines: one thread per line, lanes along k (the access shape of k_geom_lines_strided).  One walk: `carry` = the run of
// cells the walk is in has met NODE_OUT; the NODE_IN cells of the run before the first NODE_OUT (from rs on) are turned when it is met.
__global__ void __launch_bounds__(256) k_geom_fill_strided(uint8_t *type, int n_o, int dimz, long long os, long long ss, int n, unsigned *cnt)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned turned = 0;
    if (t < (long long)n_o * dimz) {
        const int o = (int)(t / dimz), k = (int)(t - (long long)o * dimz);
        uint8_t *p = type + (long long)o * os + k;
        bool carry = false;
        int rs = 0;
        for (int s0 = 0; s0 < n; s0 += 8) {               // 8 loads in flight: a wave per 64 lines leaves the memory latency uncovered
            int v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = s0 + u < n ? p[(long long)(s0 + u) * ss] : FS3D_NODE_BOUND;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int s = s0 + u, ty = v[u];              // (the walk writes no cell it has yet to look at)
                if (s >= n) break;
                if (ty == FS3D_NODE_OUT) {
                    if (!carry) { for (int q = rs; q < s; q++) p[(long long)q * ss] = FS3D_NODE_OUT; turned += s - rs; carry = true; }
                } else if (ty == FS3D_NODE_IN) {
                    if (carry) { p[(long long)s * ss] = FS3D_NODE_OUT; turned++; }
                } else { carry = false; rs = s + 1; }
            }
        }
    }
    fill_block_count(turned, cnt);
}

// 64 cells of a Z line, one per lane: a segmented scan with ballots.  A lane's run reaches from the cell after the last wall below
// it to the cell before the first wall above it; it turns when the run holds a NODE_OUT cell or touches a neighbouring chunk
// whose end cell is NODE_OUT (from_below / from_above).  Returns the turned lanes; *ends: bit 0 / 1 = the chunk's first / last cell is NODE_OUT now.
__device__ __forceinline__ unsigned long long fill_chunk(uint8_t *p, int k0, int dimz, int lane, bool from_below, bool from_above, int *ends)
{
    const int k = k0 + lane;
    const int ty = k < dimz ? p[k] : FS3D_NODE_BOUND;                  // past the line's end: a wall
    const unsigned long long wall = __ballot(ty != FS3D_NODE_IN && ty != FS3D_NODE_OUT), out = __ballot(ty == FS3D_NODE_OUT);
    const unsigned long long below = wall & ((1ull << lane) - 1), above = lane == 63 ? 0ull : wall >> (lane + 1);
    const int lo = below ? 64 - __clzll((long long)below) : 0, hi = above ? lane + __ffsll((unsigned long long)above) - 1 : 63;
    const unsigned long long run = (hi == 63 ? ~0ull : (1ull << (hi + 1)) - 1) & ~((1ull << lo) - 1);
    const bool src = (out & run) != 0 || (from_below && lo == 0) || (from_above && hi == 63);
    const bool turn = ty == FS3D_NODE_IN && src;
    if (turn) p[k] = FS3D_NODE_OUT;
    const unsigned long long turned = __ballot(turn), now = out | turned;
    *ends = (int)(now & 1) | (int)((now >> 63) & 1) << 1;
    return turned;
}

// Z lines are the contiguous axis: one wave per line (the access shape of k_geom_lines_z); a line of more than 64 cells goes chunk
// by chunk upwards with the carry of the chunk below, then downwards with the carry of the chunk above
__global__ void __launch_bounds__(256) k_geom_fill_z(uint8_t *type, long long nlines, int dimz, unsigned *cnt)
{
    const long long line = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned turned = 0;
    if (line < nlines) {                                               // whole waves
        uint8_t *p = type + line * dimz;
        const int nch = (dimz + 63) / 64;
        int ends = 0;
        for (int c = 0; c < nch; c++) turned += __popcll(fill_chunk(p, 64 * c, dimz, lane, (ends & 2) != 0, false, &ends));
        if (nch > 1) {
            ends = 0;
            for (int c = nch - 1; c >= 0; c--) turned += __popcll(fill_chunk(p, 64 * c, dimz, lane, false, (ends & 1) != 0, &ends));
        }
    }
    fill_block_count(lane == 0 ? turned : 0, cnt);
}

// The other six node arrays of a Shape3D grid from its finished type array (nodes_of in shape3d.py; FillShape3DNodes in host/Shape3D.h):
// bc_vel = bc_temp = NOSLIP, v = 0, T = 0 on NODE_BOUND and baseT elsewhere.  Store shapes of k_geom_extrude (store_nodes): V == 4
// cells per thread (dimz % 4 == 0 and the arrays aligned), V == 1 cell by cell.
// Stateless by definition: the reference's repeated Prepare_CPU leaves T = 0 on cells that once were walls, a value nothing reads
// after the layers have been initialised (the third stated deviation, host/Shape3D.h).
template <typename R, int V>
__global__ void __launch_bounds__(256) k_geom_mesh_nodes(const uint8_t *__restrict__ type, long long ncell, R baseT, uint8_t *__restrict__ bc_vel,
                                                          uint8_t *__restrict__ bc_temp, R *__restrict__ vx, R *__restrict__ vy, R *__restrict__ vz,
                                                          R *__restrict__ T)
{
    const long long l = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (l >= ncell) return;                                            // V == 4: ncell % 4 == 0
    unsigned w;
    if constexpr (V == 4) w = *(const unsigned *)(type + l); else w = type[l];
    R a0[V], aT[V];
#pragma unroll
    for (int q = 0; q < V; q++) { a0[q] = R(0); aT[q] = ((w >> (8 * q)) & 0xFF) == FS3D_NODE_BOUND ? R(0) : baseT; }
    constexpr unsigned noslip = 0x01010101u * FS3D_BC_NOSLIP;          // in every byte
    store_nodes<R, V, false>(l, 0u, noslip, noslip, a0, a0, aT, nullptr, bc_vel, bc_temp, vx, vy, vz, T);
}

// ---- walls that carry the mesh's velocity (fs3d_*_shape3d_vel) ---------------------------------------------------------------------
// The rule is wall_velocity of fs3d_voxel.h, shared with host/Shape3D.h (WallVelocity) and specified by wall_weights / wall_velocity
// of cmc_fluid_solver_amd/shape3d.py: float64 from the fp32 vertices, rounded after each operation.

// k_geom_mesh_nodes with walls that move: a NODE_BOUND cell reads its owner (k_geom_voxel_mesh<true>), gathers that triangle's
// three vertices and three velocities, evaluates the rule in float64 and stores v rounded once to R and T = wallT; every other
// cell as there.  The same two store shapes.  Wall cells are a surface: the gather is a small part of the seven arrays' traffic.
// A NODE_BOUND cell without an owner below ntri cannot come from the voxel kernel; it reads nothing and stays at rest.
// x0: the plane of the global grid that cell 0 of these arrays lies in (an x-slab; else 0) -- the vertices are in global grid
// coordinates, every index is local to the arrays.
template <typename R, int V>
__global__ void __launch_bounds__(256) k_geom_mesh_nodes_vel(const uint8_t *__restrict__ type, const unsigned *__restrict__ owner,
                                                              const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                              const float *__restrict__ wx, const float *__restrict__ wy, const float *__restrict__ wz,
                                                              const int *__restrict__ tri, unsigned ntri, long long ncell, int x0, int dimy, int dimz,
                                                              R baseT, R wallT, uint8_t *__restrict__ bc_vel, uint8_t *__restrict__ bc_temp,
                                                              R *__restrict__ vx, R *__restrict__ vy, R *__restrict__ vz, R *__restrict__ T)
{
    const long long l = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (l >= ncell) return;                                            // V == 4: ncell % 4 == 0
    unsigned w;
    if constexpr (V == 4) w = *(const unsigned *)(type + l); else w = type[l];
    R ax[V], ay[V], az[V], aT[V];
#pragma unroll
    for (int q = 0; q < V; q++) {
        const bool wall = ((w >> (8 * q)) & 0xFF) == FS3D_NODE_BOUND;
        ax[q] = R(0); ay[q] = R(0); az[q] = R(0); aT[q] = wall ? wallT : baseT;
        if (!wall) continue;
        const unsigned t = owner[l + q];
        if (t >= ntri) continue;
        const long long cell = l + q, col = cell / dimz;
        const double ck = (double)(int)(cell - col * dimz), cj = (double)(int)(col % dimy), ci = (double)(x0 + (int)(col / dimy));
        const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];      // checked by mesh_check: inside the vertex list
        const D3 q0 = {(double)px[i0] - ci, (double)py[i0] - cj, (double)pz[i0] - ck}, q1 = {(double)px[i1] - ci, (double)py[i1] - cj, (double)pz[i1] - ck},
                 q2 = {(double)px[i2] - ci, (double)py[i2] - cj, (double)pz[i2] - ck};
        const D3 u = wall_velocity(q0, q1, q2, {(double)wx[i0], (double)wy[i0], (double)wz[i0]}, {(double)wx[i1], (double)wy[i1], (double)wz[i1]},
                                   {(double)wx[i2], (double)wy[i2], (double)wz[i2]});
        ax[q] = (R)u.x; ay[q] = (R)u.y; az[q] = (R)u.z;
    }
    constexpr unsigned noslip = 0x01010101u * FS3D_BC_NOSLIP;          // in every byte
    store_nodes<R, V, false>(l, 0u, noslip, noslip, ax, ay, aT, nullptr, bc_vel, bc_temp, vx, vy, vz, T, az);
}

// ---- fresh cells: a cell that turns NODE_IN takes the mean of its fluid neighbours (fs3d_fill_fresh_cells*) ------------------------
// cmc_fluid_solver_amd/fresh_cells.py fill_fresh_cells is the definition; the kernels end with its bits.  Every cell carries one
// byte, its round tag: 0 a donor (NODE_IN before and now), 1 .. 250 the round that filled it, FRESH_UNFILLED a fresh cell (NODE_IN
// now, something else before) still waiting, FRESH_OTHER everything else.  In round r a neighbour counts iff its tag is below r, and
// a cell filled in round r gets tag r: a round reads only cells that no thread of the round writes (their tags are below r, the
// written ones hold FRESH_UNFILLED or r), tags are single bytes read and written as single bytes, the fields are filled in place --
// so a round is free of races and the order of the list is free.  The neighbours are summed in the order i-1, i+1, j-1, j+1, k-1,
// k+1, the first one starting the sum, then ONE division by (R)n: this file is compiled without contraction and with IEEE division.
#define FRESH_UNFILLED 254
#define FRESH_OTHER 255
#define FRESH_MAX_ROUNDS 250
#define FRESH_BATCH 2                                   // rounds between two looks at their counters
// counter words of one fill (unsigned): [0] the fresh cells (the list's length), [r] the cells round r filled, r = 1 .. 250
enum { FC_FRESH = 0, FC_WORDS = FRESH_MAX_ROUNDS + 2 };

typedef unsigned FreshU4 __attribute__((ext_vector_type(4)));
typedef unsigned FreshU2 __attribute__((ext_vector_type(2)));

// node types of the V == 8 cells from l (l % 8 == 0: the table is aligned to 16 bytes), one per byte of the two result words
__device__ __forceinline__ FreshU2 fresh_types8(const uint16_t *__restrict__ code, long long l)
{
    const FreshU4 cw = *(const FreshU4 *)(code + l);
    FreshU2 t = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 8; q++) t[q >> 2] |= ((cw[q >> 1] >> (16 * (q & 1) + CODE_TYPE_SHIFT)) & 3u) << (8 * (q & 3));
    return t;
}

// The snapshot of FS3D_OPT_FRESH_CELLS: the node types of the code table, one byte per cell, before an update rewrites the table.
__global__ void __launch_bounds__(256) k_fresh_snapshot(const uint16_t *__restrict__ code, long long ncell, uint8_t *__restrict__ prev)
{
    const long long l = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
    if (l + 8 <= ncell) *(FreshU2 *)(prev + l) = fresh_types8(code, l);        // (prev is the context's own allocation: aligned)
    else for (long long q = l; q < ncell; q++) prev[q] = (uint8_t)((code[q] >> CODE_TYPE_SHIFT) & 3);
}

// One streaming pass: the round tag of every cell from its code word and its previous type, and the compact list of the fresh
// cells.  One thread takes V consecutive cells -- V == 8 (prev aligned to 8 bytes): 16 bytes of codes, 8 of previous types and 8 of
// tags per access, the last cells of a grid that is no multiple of 8 one by one; V == 1: cell by cell.  The list is appended by a
// wave scan and ONE atomic per workgroup and tile (as k_geom_bnd_list); entries beyond `cap` are dropped and the host, which reads
// the count, grows the list and runs the pass again.
template <int V>
__global__ void __launch_bounds__(256) k_fresh_classify(const uint16_t *__restrict__ code, const uint8_t *__restrict__ prev, long long ncell,
                                                         uint8_t *__restrict__ tag, int *__restrict__ list, long long cap, unsigned *cnt)
{
    __shared__ unsigned s_cnt[4];
    __shared__ unsigned s_first;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long ngroup = (ncell + V - 1) / V;
    for (long long g0 = (long long)blockIdx.x * 256; g0 < ngroup; g0 += (long long)gridDim.x * 256) {      // workgroup-uniform
        const long long l0 = (g0 + threadIdx.x) * V;
        unsigned fresh = 0;                                 // bit q: cell l0 + q is fresh
        if (V == 8 && l0 + 8 <= ncell) {
            const FreshU2 t = fresh_types8(code, l0), p = *(const FreshU2 *)(prev + l0);
            FreshU2 tg = {0u, 0u};
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned t0 = (t[q >> 2] >> (8 * (q & 3))) & 0xFFu, p0 = (p[q >> 2] >> (8 * (q & 3))) & 0xFFu;
                const unsigned v = t0 != FS3D_NODE_IN ? FRESH_OTHER : (p0 == FS3D_NODE_IN ? 0u : FRESH_UNFILLED);
                tg[q >> 2] |= v << (8 * (q & 3));
                fresh |= (unsigned)(v == FRESH_UNFILLED) << q;
            }
            *(FreshU2 *)(tag + l0) = tg;
        } else {
            for (int q = 0; q < V && l0 + q < ncell; q++) {
                const int t0 = (code[l0 + q] >> CODE_TYPE_SHIFT) & 3, p0 = prev[l0 + q];
                const unsigned v = t0 != FS3D_NODE_IN ? FRESH_OTHER : (p0 == FS3D_NODE_IN ? 0u : FRESH_UNFILLED);
                tag[l0 + q] = (uint8_t)v;
                fresh |= (unsigned)(v == FRESH_UNFILLED) << q;
            }
        }
        const unsigned mine = __popc(fresh);
        unsigned incl = mine;                               // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_cnt[w] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned all = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_first = all ? atomicAdd(&cnt[FC_FRESH], all) : 0u;
        }
        __syncthreads();
        long long pos = (long long)s_first + (incl - mine);
        for (int ww = 0; ww < w; ww++) pos += s_cnt[ww];
#pragma unroll
        for (int q = 0; q < V; q++)
            if ((fresh >> q) & 1u) {
                if (pos < cap) list[pos] = (int)(l0 + q);
                pos++;
            }
        __syncthreads();                                    // s_cnt / s_first are rewritten by the next tile
    }
}

// one neighbour of a fresh cell in round `round`: counted iff it lies inside the grid and its tag is below the round
#define FRESH_TAKE(inside, off)                                                                    \
    if ((inside) && tag[l + (off)] < round) {                                                      \
        const long long m = l + (off);                                                             \
        s0 = n ? s0 + f0[m] : f0[m]; s1 = n ? s1 + f1[m] : f1[m];                                  \
        s2 = n ? s2 + f2[m] : f2[m]; s3 = n ? s3 + f3[m] : f3[m];                                  \
        n++;                                                                                       \
    }

// Round `round` over the list of fresh cells, one thread per entry.  f0 .. f3 address the first OWNED cell of the layer's fields,
// tag the first owned cell's tag.  SLAB false, a whole grid: the halo plane in front of the fields is never read, a neighbour
// outside the grid is skipped.  SLAB true, an x-slab of a group: lo / hi say that a neighbouring slab stands before / behind the
// owned planes; its boundary plane of the fields is in the layer's ghost plane and its tags in the ghost plane of the tag array
// (fs3d_comm_fill_exchange brought both), and that neighbour counts exactly as an owned one.  cnt: the cells this round filled.
template <typename R, bool SLAB>
__global__ void __launch_bounds__(256) k_fresh_round(const int *__restrict__ list, long long nlist, uint8_t *tag, int round, int dimx,
                                                      int dimy, int dimz, R *f0, R *f1, R *f2, R *f3, unsigned *cnt, int lo, int hi)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool did = false;
    if (t < nlist) {
        const long long l = list[t];
        if (tag[l] == FRESH_UNFILLED) {
            const long long plane = (long long)dimy * dimz;
            const int i = (int)(l / plane), rem = (int)(l - (long long)i * plane), j = rem / dimz, k = rem - j * dimz;
            int n = 0;
            R s0 = R(0), s1 = R(0), s2 = R(0), s3 = R(0);
            FRESH_TAKE(i >= 1 || (SLAB && lo), -plane)
            FRESH_TAKE(i + 1 < dimx || (SLAB && hi), plane)
            FRESH_TAKE(j >= 1, -(long long)dimz)
            FRESH_TAKE(j + 1 < dimy, (long long)dimz)
            FRESH_TAKE(k >= 1, -1LL)
            FRESH_TAKE(k + 1 < dimz, 1LL)
            if (n) {
                const R d = (R)n;
                f0[l] = s0 / d; f1[l] = s1 / d; f2[l] = s2 / d; f3[l] = s3 / d;
                tag[l] = (uint8_t)round;
                did = true;
            }
        }
    }
    const unsigned long long m = __ballot(did);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt, (unsigned)__popcll(m));
}

// The collective fill: the counts of n (1 or 2) consecutive counter words as the two doubles fs3d_comm_allreduce_sum2 sums
__global__ void k_fresh_counts(const unsigned *__restrict__ cnt, int n, double *__restrict__ red)
{
    if (threadIdx.x < 2) red[threadIdx.x] = (int)threadIdx.x < n ? (double)cnt[threadIdx.x] : 0.0;
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------

// The lines of direction d.  d = 0 (X) and 1 (Y): n_o * dimz lines -- `os` apart along the outer index, neighbours along k -- of n
// cells `ss` apart; d = 2 (Z): dimx * dimy lines of dimz contiguous cells, one behind the other (n_o is not used).
struct GeomLines { int n_o; long long os, ss; int n; long long nlines; };
static inline GeomLines geom_lines(const fs3d_ctx *c, int d)
{
    if (d == 0) return {c->dimy, (long long)c->dimz, c->plane, c->dimx, (long long)c->dimy * c->dimz};
    if (d == 1) return {c->dimx, c->plane, (long long)c->dimz, c->dimy, (long long)c->dimx * c->dimz};
    return {0, (long long)c->dimz, 1, c->dimz, (long long)c->dimx * c->dimy};
}
// the same for the GLOBAL grid the context is a slab of (the flood fill of a mesh; a single context: geom_lines)
static inline GeomLines geom_lines_global(const fs3d_ctx *c, int d)
{
    const int gx = c->dimx_global;
    if (d == 0) return {c->dimy, (long long)c->dimz, c->plane, gx, (long long)c->dimy * c->dimz};
    if (d == 1) return {gx, c->plane, (long long)c->dimz, c->dimy, (long long)gx * c->dimz};
    return {0, (long long)c->dimz, 1, c->dimz, (long long)gx * c->dimy};
}
// groups of 32 k: the shared columns of directions 0 and 1 are n_o * geom_ng of them
static inline int geom_ng(const fs3d_ctx *c) { return (c->dimz + 31) / 32; }

// Device time of an update, while fs3d_enable_timing is on: an event before the first launch of every batch and one before the
// synchronisation that ends it (the host's work between two batches is not device time).
static void gev_fold(fs3d_geom &g)
{
    for (int k = 0; k + 1 < g.ev_n; k += 2) {
        float ms = 0;
        if (hipEventSynchronize(g.ev[k + 1]) == hipSuccess && hipEventElapsedTime(&ms, g.ev[k], g.ev[k + 1]) == hipSuccess) g.ev_ms += ms;
    }
    g.ev_n = 0;
}
static void gev_begin(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    if (!c->timing_period || g.ev_open) return;
    if (g.ev_n + 2 > 16) gev_fold(g);                  // (the flood fill of a mesh has one batch per look at its counters)
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
static void gev_reset(fs3d_ctx *c) { c->geom.ev_n = 0; c->geom.ev_open = false; c->geom.ev_ms = 0; }
static void gev_collect(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    gev_end(c);
    gev_fold(g);
    g.last_dev_ms = g.ev_ms;
    g.ev_ms = 0;
}

// ends a batch: the event that closes it, then the wait for the stream
static fs3d_status gev_sync(fs3d_ctx *c)
{
    gev_end(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}
// the device time gathered since gev_reset, for a caller that is no update (fs3d_last_update_device_ms keeps its value)
static float gev_take(fs3d_ctx *c)
{
    fs3d_geom &g = c->geom;
    gev_end(c);
    gev_fold(g);
    const float ms = g.ev_ms;
    g.ev_ms = 0;
    return ms;
}

// (the buffers of fs3d_geom go with the context)
void fs3d_geom_destroy(fs3d_ctx *c) { for (hipEvent_t e : c->geom.ev) if (e) hipEventDestroy(e); }

// cells of the global grid: the byte arrays of an update cover them (a single context: its own cells)
static inline long long geom_gcell(const fs3d_ctx *c) { return (long long)c->dimx_global * c->plane; }

// the buffers an update keeps: allocated by the first one
static fs3d_status geom_prepare(fs3d_ctx *c, bool need_stage)
{
    fs3d_geom &g = c->geom;
    long long *const na = &c->geom_allocs;
    if (need_stage) BUFCHK(c, g.stage.reserve((size_t)3 * geom_gcell(c), na));      // (an x-slab: the byte arrays of the global grid)
    for (int d = 0; d < 3; d++) BUFCHK(c, g.lst[d].reserve((size_t)geom_lines(c, d).nlines * sizeof(int), na));
    size_t host_bytes = GC_WORDS * sizeof(unsigned long long);
    for (int d = 0; d < 2; d++) {
        const GeomLines L = geom_lines(c, d);
        if (L.n > UCOL_PITCH) continue;                  // as geom_shared_columns: no shared columns for longer lines
        const size_t nq = (size_t)L.n_o * geom_ng(c);
        bool fresh = false;
        BUFCHK(c, g.col[d].reserve(nq * UCOL_PITCH * sizeof(uint16_t), na, &fresh));
        if (fresh) HIPCHK(c, hipMemsetAsync(g.col[d], 0, nq * UCOL_PITCH * sizeof(uint16_t), c->stream));
        BUFCHK(c, g.cflag[d].reserve(nq, na));
        BUFCHK(c, g.hash[d].reserve(nq * sizeof(unsigned long long), na));
        BUFCHK(c, g.rep[d].reserve(nq * sizeof(int), na));
        host_bytes = std::max(host_bytes, nq * (sizeof(unsigned long long) + sizeof(unsigned) + sizeof(int) + 1) + 64);
    }
    BUFCHK(c, g.host.reserve(host_bytes));
    BUFCHK(c, g.cnt.reserve(GC_WORDS * sizeof(unsigned long long), na));
    return FS3D_OK;
}

// shared columns of direction d from the new code table (dead[d] is current)
static fs3d_status geom_columns(fs3d_ctx *c, int d)
{
    fs3d_geom &g = c->geom;
    const GeomLines L = geom_lines(c, d);
    const int ng = geom_ng(c);
    if (L.n > UCOL_PITCH) { c->n_ucol[d] = 0; return FS3D_OK; }
    const size_t nq = (size_t)L.n_o * ng;
    if (c->ucol_cap[d] < (long long)nq) {                // the upload's table holds its own distinct columns only: once, room for any number
        c->ucol_cap[d] = 0;
        BUFCHK(c, c->ucol[d].replace(nq * UCOL_PITCH * sizeof(uint16_t), &c->geom_allocs));
        c->ucol_cap[d] = (long long)nq;
    }
    const int keep = (0xF << (4 * d)) | (3 << CODE_TYPE_SHIFT);
    gev_begin(c);
    hipLaunchKernelGGL(k_geom_columns, dim3((unsigned)(L.n_o * ((ng + 1) / 2))), dim3(64), 0, c->stream, c->code, c->dead[d], ng, c->dimz,
                       L.os, L.ss, L.n, keep, g.col[d], g.cflag[d], g.hash[d]);
    HIPCHK(c, hipGetLastError());
    // identities on the host from the hashes (a few KB), numbered in the order of first appearance as geom_shared_columns numbers them
    unsigned long long *hh = (unsigned long long *)g.host;
    unsigned *fl = (unsigned *)(hh + nq);
    int *rep = (int *)(fl + nq);
    uint8_t *cf = (uint8_t *)(rep + nq);
    HIPCHK(c, hipMemcpyAsync(hh, g.hash[d], nq * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cf, g.cflag[d], nq, hipMemcpyDeviceToHost, c->stream));
    GTRY(gev_sync(c));
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
    HIPCHK(c, hipMemcpyAsync(c->uflag[d], fl, nq * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    if (nid) {
        HIPCHK(c, hipMemcpyAsync(g.rep[d], rep, nid * sizeof(int), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_geom_gather, dim3(nid), dim3(256), 0, c->stream, g.col[d], g.rep[d], c->ucol[d]);
        hipLaunchKernelGGL(k_geom_verify, dim3((unsigned)nq), dim3(64), 0, c->stream, g.col[d], c->uflag[d], c->ucol[d], L.n, g.cnt);
        HIPCHK(c, hipGetLastError());
    }
    // the pinned block is reused by the next direction: its copies must have left
    return gev_sync(c);
}

// The three byte arrays cover the global grid; the tables are those of the context's planes.  slab (fs3d_update_nodes*_slab): the
// X lines are read from the global arrays (k_geom_lines_x_slab, k_geom_codes<true>); everything else runs on the local planes.
// Without it the context is the whole grid (the other entries refuse a slab) and line and context coincide.
// name: the entry that was called; the refusals of a slab entry carry it, those of a whole-grid entry say fs3d_update_nodes.
template <typename R>
static fs3d_status update_nodes_impl(fs3d_ctx *c, const uint8_t *gtype, const uint8_t *gbc_vel, const uint8_t *gbc_temp, const char *entry,
                                     bool slab, int n_seg_out[3])
{
    fs3d_geom &g = c->geom;
    const long long ncell = c->ncell, first = (long long)c->x_offset * c->plane;
    const uint8_t *type = gtype + first, *bc_vel = gbc_vel + first, *bc_temp = gbc_temp + first;
    const std::string name = slab ? entry : "fs3d_update_nodes";
    HIPCHK(c, hipMemsetAsync(g.cnt, 0, GC_WORDS * sizeof(unsigned long long), c->stream));
    for (int d = 0; d < 3; d++) {
        const GeomLines L = geom_lines(c, d);
        if (d == 0 && slab)
            hipLaunchKernelGGL(k_geom_lines_x_slab, dim3(grid_for(L.nlines, 1 << 30)), dim3(256), 0, c->stream, gtype, gbc_vel, gbc_temp,
                               L.nlines, L.ss, c->dimx_global, c->x_offset, c->dimx, g.lst[d], c->dead[d], g.cnt);
        else if (d < 2)
            hipLaunchKernelGGL(k_geom_lines_strided, dim3(grid_for(L.nlines, 1 << 30)), dim3(256), 0, c->stream, type, L.n_o, c->dimz,
                               L.os, L.ss, L.n, g.lst[d], c->dead[d]);
        else
            hipLaunchKernelGGL(k_geom_lines_z, dim3(grid_for(L.nlines * 64, 1 << 30)), dim3(256), 0, c->stream, type, L.nlines, c->dimz,
                               g.lst[d], c->dead[d]);
    }
    hipLaunchKernelGGL(slab ? k_geom_codes<true> : k_geom_codes<false>, dim3(grid_for(ncell)), dim3(256), 0, c->stream, type, bc_vel, bc_temp,
                       g.lst[0], g.lst[1], g.lst[2], c->dimx, c->dimy, c->dimz, c->x_offset, c->dimx_global, c->code, g.cnt);
    HIPCHK(c, hipGetLastError());
    unsigned long long *hc = (unsigned long long *)g.host;
    HIPCHK(c, hipMemcpyAsync(hc, g.cnt, GC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    GTRY(gev_sync(c));
    if (hc[GC_SHARED])
        return fail(c, FS3D_ERR_UNSUPPORTED,
                     name + ": a cell with a FREE boundary condition closes one segment and opens the next "
                     "on the same line (two rows on one cell; the reference's result there depends on thread timing)");
    const long long nseg[3] = {(long long)hc[0], (long long)hc[1], (long long)hc[2]};
    const long long nbnd = (long long)hc[GC_NBND];
    c->stale_in_cells = (long long)hc[GC_STALE];
    // BOUND / VALVE list: grow-only
    if (nbnd > c->bnd_cap) {
        c->bnd_cap = 0; c->n_bnd = 0;
        const long long cap = std::min<long long>(ncell, nbnd + nbnd / 4 + 1024);      // headroom: the list of a moving wall breathes
        BUFCHK(c, c->bnd_idx.replace(sizeof(int) * (size_t)cap, &c->geom_allocs));
        for (int v = 0; v < 4; v++) BUFCHK(c, c->bnd_val[v].replace(sizeof(R) * (size_t)cap, &c->geom_allocs));
        c->bnd_cap = (int)cap;
    }
    if (nbnd) {
        gev_begin(c);
        hipLaunchKernelGGL((k_geom_bnd_list<R>), dim3(grid_for((ncell + GEOM_LIST_CHUNKS - 1) / GEOM_LIST_CHUNKS)), dim3(256), 0, c->stream, type, ncell, (const R *)c->node,
                           c->nstride, c->bnd_cap, c->bnd_idx, (R *)c->bnd_val[0], (R *)c->bnd_val[1], (R *)c->bnd_val[2],
                           (R *)c->bnd_val[3], g.cnt);
        HIPCHK(c, hipGetLastError());
    }
    for (int d = 0; d < 2; d++) GTRY(geom_columns(c, d));
    gev_begin(c);
    HIPCHK(c, hipMemcpyAsync(hc, g.cnt, GC_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    GTRY(gev_sync(c));
    if ((long long)hc[GC_LIST] != nbnd)
        return fail(c, FS3D_ERR_HIP, name + ": the BOUND / VALVE list does not hold the counted cells");
    if (hc[GC_MISMATCH])
        return fail(c, FS3D_ERR_HIP, name + ": two different shared code columns have the same hash; tables not usable");
    c->n_bnd = (int)nbnd;
    for (int d = 0; d < 3; d++) { c->nseg[d] = (int)nseg[d]; if (n_seg_out) n_seg_out[d] = (int)nseg[d]; }
    return FS3D_OK;
}

// ---- the seven node arrays on the device, as the extrusion and the voxelisation write them --------------------------------------
struct NodeArrays {
    uint8_t *type, *bc_vel, *bc_temp;
    void *v[4];                                         // vx, vy, vz, T in the context's precision
    bool any_null() const { return !type || !bc_vel || !bc_temp || !v[0] || !v[1] || !v[2] || !v[3]; }
    // V == 4 of the two node-writing kernels: dimz % 4 == 0, the byte arrays aligned to 4 bytes and the value arrays to 16
    bool vec4(int dimz) const
    {
        uintptr_t mis = ((uintptr_t)type | (uintptr_t)bc_vel | (uintptr_t)bc_temp) & 3;
        mis |= ((uintptr_t)v[0] | (uintptr_t)v[1] | (uintptr_t)v[2] | (uintptr_t)v[3]) & 15;
        return dimz % 4 == 0 && !mis;
    }
};

// the context's own: the three byte arrays (of the global grid) in the staging buffer, the four value fields (of its planes) in
// place in the node-value table
static NodeArrays geom_own_arrays(const fs3d_ctx *c)
{
    uint8_t *sg = c->geom.stage;
    const long long gcell = sg ? geom_gcell(c) : 0;      // (no staging buffer: fs3d_update_nodes_dev, which reads its own byte arrays)
    NodeArrays a = {sg, sg + gcell, sg + 2 * gcell, {}};
    for (int v = 0; v < 4; v++) a.v[v] = (char *)c->node + (size_t)v * c->nstride * c->esize;
    return a;
}

// ---- extrusion of a Shape2D grid ----------------------------------------------------------------------------------------------
struct ExtrudeIn {
    const uint8_t *cell; const float *velx, *vely, *T; double dz, depth, depth_var, baseT; int A = 0;      // A: extrude_check's
    bool any_null() const { return !cell || !velx || !vely || !T; }
};

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
        return fail(c, FS3D_ERR_INVALID, std::string(name) + ": active_dimz = ceil(depth / dz) + 1 must lie in 2 .. dimz");
    const size_t ncol = (size_t)c->dimx_global * c->dimy;      // the 2D grid covers the global plane (a single context: its own)
    HIPCHK(c, hipSetDevice(c->device));
    BUFCHK(c, g.ex_host.reserve(ex_bytes(ncol)));
    bool fresh = false;                                   // (a failure leaves the buffer empty: the next call allocates again)
    BUFCHK(c, g.ex_dev.reserve(ex_bytes(ncol), &c->geom_allocs, &fresh));
    if (fresh) { g.ex_bottom_valid = false; g.ex_dz = -1; }
    char *h = (char *)g.ex_host;
    int *bottom = (int *)(h + ex_off_bottom(ncol));
    if (g.ex_dz != in.dz || g.ex_depth != in.depth || g.ex_depth_var != in.depth_var) {      // (a NaN depth_var: recomputed every call)
        extrude_bottom_table(c->dimx_global, c->dimy, in.A, in.depth_var, bottom);
        g.ex_dz = in.dz; g.ex_depth = in.depth; g.ex_depth_var = in.depth_var; g.ex_bottom_valid = false;
    }
    for (size_t q = 0; q < ncol; q++) {
        const uint8_t t = in.cell[q];
        if (t > FS3D_NODE_VALVE) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": a cell2d value is not a node type");
        // where ExtrudeShape2D would write outside the column's dimz cells (it reads `bottom` of the columns that are not NODE_OUT)
        if (t != FS3D_NODE_OUT && (bottom[q] < -1 || bottom[q] >= c->dimz))
            return fail(c, FS3D_ERR_INVALID, std::string(name) + ": depth_var puts the bottom of a column outside the grid");
    }
    memcpy(h, in.velx, 4 * ncol); memcpy(h + 4 * ncol, in.vely, 4 * ncol); memcpy(h + 8 * ncol, in.T, 4 * ncol);
    memcpy(h + ex_off_cell(ncol), in.cell, ncol);
    return FS3D_OK;
}

// the column records to the device and the kernel, on the context's stream; not synchronised.  slab: the byte arrays of `a` cover
// the global grid, its value arrays the context's planes (k_geom_extrude<.., true>); else all seven cover the same cells.
template <typename R>
static fs3d_status extrude_launch(fs3d_ctx *c, const ExtrudeIn &in, const NodeArrays &a, bool slab)
{
    fs3d_geom &g = c->geom;
    const size_t ncol = (size_t)c->dimx_global * c->dimy;
    const char *d = (const char *)g.ex_dev;
    HIPCHK(c, hipMemcpyAsync(g.ex_dev, g.ex_host, g.ex_bottom_valid ? ex_off_cell(ncol) + ncol : ex_bytes(ncol), hipMemcpyHostToDevice, c->stream));
    g.ex_bottom_valid = true;
    const bool vec = a.vec4(c->dimz);
    const long long nthr = (long long)ncol * (vec ? c->dimz / 4 : c->dimz);
    auto kern = slab ? (vec ? k_geom_extrude<R, 4, true> : k_geom_extrude<R, 1, true>) : (vec ? k_geom_extrude<R, 4, false> : k_geom_extrude<R, 1, false>);
    hipLaunchKernelGGL(kern, dim3(grid_for(nthr, 1 << 30)), dim3(256), 0, c->stream, (const float *)d, (const float *)(d + 4 * ncol),
                       (const float *)(d + 8 * ncol), (const int *)(d + ex_off_bottom(ncol)), (const uint8_t *)(d + ex_off_cell(ncol)),
                       (long long)ncol, (long long)c->x_offset * c->dimy, (long long)c->dimx * c->dimy, c->dimz, in.A, (float)in.baseT,
                       a.type, a.bc_vel, a.bc_temp, (R *)a.v[0], (R *)a.v[1], (R *)a.v[2], (R *)a.v[3]);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

// ---- voxelisation of a Shape3D mesh ---------------------------------------------------------------------------------------------
// vel: an entry with wall velocities -- wx, wy, wz per vertex and the walls' temperature (else null and 0)
struct MeshIn {
    const float *x, *y, *z; int nvert; const int *tri; int ntri; double baseT;
    bool vel = false; const float *wx = nullptr, *wy = nullptr, *wz = nullptr; double wallT = 0.0;
    bool any_null() const { return !x || !y || !z || !tri || (vel && (!wx || !wy || !wz)); }
};
#define MESH_COLS 6                                    // columns of mesh_vcap floats in the pinned and the device block: x, y, z, wx, wy, wz

#define MESH_FILL_BATCH 2                              // rounds of the flood fill between two looks at their counters
enum { MC_FLAG = 0, MC_ROUND = 1, MC_WORDS = 1 + MESH_FILL_BATCH };

static inline float *mesh_host_vert(const fs3d_geom &g) { return (float *)g.mesh_host; }
static inline int *mesh_host_idx(const fs3d_geom &g) { return (int *)((float *)g.mesh_host + MESH_COLS * (size_t)g.mesh_vcap); }
static inline unsigned *mesh_host_cnt(const fs3d_geom &g) { return (unsigned *)(mesh_host_idx(g) + 3 * (size_t)g.mesh_tcap); }

// the buffers of the mesh paths, for at least nvert vertices and ntri triangles: allocated by the first call, grown by a larger mesh.
// The velocity columns have their room beside the vertex columns from the start (the number of allocations is the same with and
// without them); the owner array, 4 bytes per cell, is allocated by the first call of an entry with wall velocities.
static fs3d_status mesh_prepare(fs3d_ctx *c, int nvert, int ntri, bool vel = false)
{
    fs3d_geom &g = c->geom;
    HIPCHK(c, hipSetDevice(c->device));
    BUFCHK(c, g.mesh_cnt.reserve(MC_WORDS * sizeof(unsigned), &c->geom_allocs));
    if (vel) BUFCHK(c, g.mesh_owner.reserve((size_t)c->ncell * sizeof(unsigned), &c->geom_allocs));
    if (g.mesh_host && g.mesh_vert && g.mesh_idx && nvert <= g.mesh_vcap && ntri <= g.mesh_tcap) return FS3D_OK;
    // either capacity exceeded: the pinned block and both device copies are made again together
    g.mesh_vcap = std::max(std::max(nvert, g.mesh_vcap), 1); g.mesh_tcap = std::max(std::max(ntri, g.mesh_tcap), 1); g.mesh_ntri_dev = -1;
    BUFCHK(c, g.mesh_host.replace((MESH_COLS * (size_t)g.mesh_vcap + 3 * (size_t)g.mesh_tcap) * 4 + MC_WORDS * sizeof(unsigned)));
    BUFCHK(c, g.mesh_vert.replace(MESH_COLS * (size_t)g.mesh_vcap * sizeof(float), &c->geom_allocs));
    BUFCHK(c, g.mesh_idx.replace(3 * (size_t)g.mesh_tcap * sizeof(int), &c->geom_allocs));
    return FS3D_OK;
}

// Everything that refuses a mesh, before anything is launched; leaves the vertices (and new indices) in the pinned block.
// *new_idx: the index list differs from the one on the device.
static fs3d_status mesh_check(fs3d_ctx *c, const MeshIn &in, const char *name, bool *new_idx)
{
    fs3d_geom &g = c->geom;
    const bool conservative = c->opt_mesh_voxels == 1;
    if (in.vel && !conservative)                         // the owner of a wall cell is defined by the conservative overlap test
        return fail(c, FS3D_ERR_INVALID, std::string(name) + ": wall velocities need the conservative voxelisation (FS3D_OPT_MESH_VOXELS = 1)");
    if (c->opt_mesh_shell && !conservative)              // the thin shell is a filter inside the conservative overlap test
        return fail(c, FS3D_ERR_INVALID, std::string(name) + ": the thin shell (FS3D_OPT_MESH_SHELL = 1) needs the conservative voxelisation (FS3D_OPT_MESH_VOXELS = 1)");
    if (in.nvert < 1 || in.ntri < 0) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": a mesh has at least one vertex and no negative number of triangles");
    for (int q = 0; q < 3 * in.ntri; q++)
        if (in.tri[q] < 0 || in.tri[q] >= in.nvert) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": triangle index outside the vertex list");
    // keeps (int) defined and the line loops short
    for (const float *a : {in.x, in.y, in.z})
        for (int q = 0; q < in.nvert; q++)
            if (!(std::fabs(a[q]) <= (conservative ? VOXEL_COORD_MAX : 65536.0f)))
                return fail(c, FS3D_ERR_INVALID, std::string(name) + (conservative
                             ? ": a vertex coordinate is not finite or exceeds 4096 grid cells in magnitude (the bound of the conservative voxelisation's slack)"
                             : ": a vertex coordinate is not finite or exceeds 65536 grid cells in magnitude"));
    if (in.vel) {
        if (!std::isfinite((float)in.wallT)) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": the wall temperature is not finite (as a float, like baseT)");
        for (const float *a : {in.wx, in.wy, in.wz})
            for (int q = 0; q < in.nvert; q++)
                if (!std::isfinite(a[q])) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": a vertex velocity is not finite");
    }
    GTRY(mesh_prepare(c, in.nvert, in.ntri, in.vel));
    float *hv = mesh_host_vert(g);
    memcpy(hv, in.x, 4 * (size_t)in.nvert); memcpy(hv + g.mesh_vcap, in.y, 4 * (size_t)in.nvert); memcpy(hv + 2 * (size_t)g.mesh_vcap, in.z, 4 * (size_t)in.nvert);
    if (in.vel) {
        memcpy(hv + 3 * (size_t)g.mesh_vcap, in.wx, 4 * (size_t)in.nvert); memcpy(hv + 4 * (size_t)g.mesh_vcap, in.wy, 4 * (size_t)in.nvert);
        memcpy(hv + 5 * (size_t)g.mesh_vcap, in.wz, 4 * (size_t)in.nvert);
    }
    *new_idx = g.mesh_ntri_dev != in.ntri || memcmp(mesh_host_idx(g), in.tri, 12 * (size_t)in.ntri) != 0;
    if (*new_idx) memcpy(mesh_host_idx(g), in.tri, 12 * (size_t)in.ntri);
    return FS3D_OK;
}

// FloodFill on a device type array of the GLOBAL grid (a single context: its own), on the context's stream; returns synchronised.  with_flag: the rasteriser ran before on the
// same counters -- its flag word comes back with the first batch of rounds.  Every batch of rounds is a batch of the device time
// (the first one goes on with the caller's, where one is open) and ends closed: what the caller launches next begins its own.
static fs3d_status mesh_fill(fs3d_ctx *c, uint8_t *type, bool with_flag, const char *name)
{
    fs3d_geom &g = c->geom;
    unsigned *hc = mesh_host_cnt(g);
    HIPCHK(c, hipMemsetAsync(type, FS3D_NODE_OUT, 1, c->stream));      // cell (0,0,0), whatever it was
    g.mesh_fill_rounds = 0;
    // no cap on the rounds: one that changes nothing ends the fill, every other one turns at least one cell
    for (bool first = true, done = false; !done; first = false) {
        gev_begin(c);
        HIPCHK(c, hipMemsetAsync(g.mesh_cnt + MC_ROUND, 0, MESH_FILL_BATCH * sizeof(unsigned), c->stream));
        for (int r = 0; r < MESH_FILL_BATCH; r++)
            for (int d = 2; d >= 0; d--) {
                const GeomLines L = geom_lines_global(c, d);   // the fill is global: a slab's own lines would stop at its cuts
                unsigned *cnt = g.mesh_cnt + MC_ROUND + r;
                if (d == 2)
                    hipLaunchKernelGGL(k_geom_fill_z, dim3(grid_for(L.nlines * 64, 1 << 30)), dim3(256), 0, c->stream, type, L.nlines, c->dimz, cnt);
                else
                    hipLaunchKernelGGL(k_geom_fill_strided, dim3(grid_for(L.nlines, 1 << 30)), dim3(256), 0, c->stream, type, L.n_o, c->dimz,
                                       L.os, L.ss, L.n, cnt);
            }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(hc, g.mesh_cnt, MC_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        GTRY(gev_sync(c));
        if (first && with_flag && hc[MC_FLAG])
            return fail(c, FS3D_ERR_INVALID, std::string(name) + (hc[MC_FLAG] & MESH_FLAG_SCANLINE
                         ? ": Shape3D: a scan line of a polygon never reaches its end cell (the reference loops there)"
                         : ": Shape3D: the scan of a polygon stops advancing (its triangle is too thin for fp32 at these coordinates; the reference loops there)"));
        for (int r = 0; r < MESH_FILL_BATCH && !done; r++) { g.mesh_fill_rounds++; done = hc[MC_ROUND + r] == 0; }
    }
    return FS3D_OK;
}

// vertices (and new indices) to the device, raster, fill and node kernels into the seven arrays, on the context's stream; the
// node kernel is not waited for.  On an x-slab (the slab entries; every other caller has refused one) the three byte arrays of `a`
// cover the GLOBAL grid and the value arrays the context's planes, as geom_own_arrays gives them: raster and fill run over the
// global grid -- every rank repeats them and talks to nobody -- bc_vel / bc_temp are NOSLIP on all global cells, and the node
// kernel works on the slab's planes.  A single context is the case x_offset == 0, dimx_global == dimx of the same lines.
template <typename R>
static fs3d_status mesh_launch(fs3d_ctx *c, const MeshIn &in, bool new_idx, const char *name, const NodeArrays &a)
{
    fs3d_geom &g = c->geom;
    HIPCHK(c, hipMemcpyAsync(g.mesh_vert, g.mesh_host, (in.vel ? MESH_COLS : 3) * (size_t)g.mesh_vcap * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (new_idx) {
        g.mesh_ntri_dev = -1;
        HIPCHK(c, hipMemcpyAsync(g.mesh_idx, mesh_host_idx(g), 12 * (size_t)std::max(in.ntri, 1), hipMemcpyHostToDevice, c->stream));
        g.mesh_ntri_dev = in.ntri;
    }
    const long long gcell = geom_gcell(c), first = (long long)c->x_offset * c->plane, tail = gcell - first - c->ncell;
    const int gx = c->dimx_global;
    HIPCHK(c, hipMemsetAsync(a.type, FS3D_NODE_IN, (size_t)gcell, c->stream));
    HIPCHK(c, hipMemsetAsync(g.mesh_cnt, 0, sizeof(unsigned), c->stream));
    const bool conservative = c->opt_mesh_voxels == 1;      // (mesh_check admitted the coordinates for this mode)
    if (in.vel) HIPCHK(c, hipMemsetAsync(g.mesh_owner, 0xFF, (size_t)c->ncell * sizeof(unsigned), c->stream));      // (the entries admit conservative only)
    const bool thin = c->opt_mesh_shell == 1;               // (mesh_check admitted it with the conservative mode only)
    auto vox_own = thin ? k_geom_voxel_mesh<true, true> : k_geom_voxel_mesh<true, false>;
    auto vox = thin ? k_geom_voxel_mesh<false, true> : k_geom_voxel_mesh<false, false>;
    if (in.ntri && in.vel)
        hipLaunchKernelGGL(vox_own, dim3((unsigned)in.ntri), dim3(64), 0, c->stream, g.mesh_vert, g.mesh_vert + g.mesh_vcap,
                           g.mesh_vert + 2 * (size_t)g.mesh_vcap, g.mesh_idx, gx, c->dimy, c->dimz, a.type, g.mesh_owner, c->x_offset, c->dimx);
    else if (in.ntri && conservative)
        hipLaunchKernelGGL(vox, dim3((unsigned)in.ntri), dim3(64), 0, c->stream, g.mesh_vert, g.mesh_vert + g.mesh_vcap,
                           g.mesh_vert + 2 * (size_t)g.mesh_vcap, g.mesh_idx, gx, c->dimy, c->dimz, a.type, (unsigned *)nullptr, 0, 0);
    else if (in.ntri)
        hipLaunchKernelGGL(k_geom_raster_mesh, dim3((unsigned)in.ntri), dim3(64), 0, c->stream, g.mesh_vert, g.mesh_vert + g.mesh_vcap,
                           g.mesh_vert + 2 * (size_t)g.mesh_vcap, g.mesh_idx, gx, c->dimy, c->dimz, a.type, g.mesh_cnt + MC_FLAG);
    HIPCHK(c, hipGetLastError());
    GTRY(mesh_fill(c, a.type, !conservative, name));        // the conservative kernel has no flag word: it stays zero
    gev_begin(c);
    // the planes of the other slabs: bytes only (their cells are on this slab's X lines)
    for (uint8_t *b : {a.bc_vel, a.bc_temp}) {
        if (first) HIPCHK(c, hipMemsetAsync(b, FS3D_BC_NOSLIP, (size_t)first, c->stream));
        if (tail) HIPCHK(c, hipMemsetAsync(b + first + c->ncell, FS3D_BC_NOSLIP, (size_t)tail, c->stream));
    }
    const NodeArrays s = {a.type + first, a.bc_vel + first, a.bc_temp + first, {a.v[0], a.v[1], a.v[2], a.v[3]}};      // the context's planes
    const bool vec = s.vec4(c->dimz);                       // (first is a multiple of dimz)
    if (in.vel) {
        auto kv = vec ? k_geom_mesh_nodes_vel<R, 4> : k_geom_mesh_nodes_vel<R, 1>;
        const float *v = g.mesh_vert;
        const size_t cap = (size_t)g.mesh_vcap;
        hipLaunchKernelGGL(kv, dim3(grid_for(vec ? c->ncell / 4 : c->ncell, 1 << 30)), dim3(256), 0, c->stream, s.type, g.mesh_owner, v, v + cap,
                           v + 2 * cap, v + 3 * cap, v + 4 * cap, v + 5 * cap, g.mesh_idx, (unsigned)in.ntri, c->ncell, c->x_offset, c->dimy, c->dimz,
                           (R)(float)in.baseT, (R)(float)in.wallT, s.bc_vel, s.bc_temp, (R *)s.v[0], (R *)s.v[1], (R *)s.v[2], (R *)s.v[3]);
        HIPCHK(c, hipGetLastError());
        return FS3D_OK;
    }
    auto kern = vec ? k_geom_mesh_nodes<R, 4> : k_geom_mesh_nodes<R, 1>;
    hipLaunchKernelGGL(kern, dim3(grid_for(vec ? c->ncell / 4 : c->ncell, 1 << 30)), dim3(256), 0, c->stream, s.type, c->ncell, (R)(float)in.baseT,
                       s.bc_vel, s.bc_temp, (R *)s.v[0], (R *)s.v[1], (R *)s.v[2], (R *)s.v[3]);
    HIPCHK(c, hipGetLastError());
    return FS3D_OK;
}

static bool geom_is_slab(const fs3d_ctx *c) { return c->dimx != c->dimx_global || c->x_offset != 0 || c->comm || c->local || c->nranks > 1; }
// FS3D_OPT_FRESH_CELLS_SLABS on a member of a group: the slab keeps the snapshot and the fill is the collective one
static bool fresh_collective(const fs3d_ctx *c) { return c->opt_fresh_slabs && (c->local || c->comm); }

// The refusals every geometry entry begins with, in this order.  slab_what: the entry's own wording of its refusal of a slab
// ("moving geometry is", ...); null: the entry takes a slab.
static fs3d_status geom_refuse(fs3d_ctx *c, const char *name, bool any_null, const char *slab_what)
{
    if (!c) return FS3D_ERR_INVALID;
    if (any_null) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": NULL array");
    if (slab_what && geom_is_slab(c))
        return fail(c, FS3D_ERR_UNSUPPORTED, std::string(name) + ": " + slab_what + " implemented for a single context only, "
                     "not for an x-slab of a larger grid or a member of a multi-GPU group");
    return FS3D_OK;
}

// FS3D_OPT_FRESH_CELLS: the node types of the code table into the snapshot, before the update that called rewrites the table.
// *taken: the context had a geometry to take them from (after a failed update it has none).  Its device time is kept apart from
// the update's and counted with the fill that reads the snapshot (fs3d_last_fill_device_ms).
static fs3d_status fresh_snapshot(fs3d_ctx *c, bool *taken)
{
    fs3d_geom &g = c->geom;
    *taken = false;
    g.prev_valid = false; g.snap_ms = 0;
    BUFCHK(c, g.prev_type.reserve((size_t)c->ncell, &c->geom_allocs));
    if (!c->have_nodes) return FS3D_OK;
    gev_reset(c);
    gev_begin(c);
    hipLaunchKernelGGL(k_fresh_snapshot, dim3(grid_for((c->ncell + 7) / 8, 1 << 30)), dim3(256), 0, c->stream, c->code, c->ncell, g.prev_type);
    HIPCHK(c, hipGetLastError());
    g.snap_ms = gev_take(c);
    *taken = true;
    return FS3D_OK;
}

// ---- fs3d_update_nodes*: one update ---------------------------------------------------------------------------------------------
typedef std::chrono::steady_clock::time_point geom_clock;

// rebuilt in place: from here until the end of update_end the context has no geometry.  Opens the first batch of the device time.
static fs3d_status update_begin(fs3d_ctx *c, bool need_stage)
{
    c->have_nodes = false;
    GTRY(geom_prepare(c, need_stage));
    gev_reset(c);
    gev_begin(c);
    return FS3D_OK;
}

// The tables from the byte arrays (the value fields are in the node-value table by now), the device time and the CreateSegments
// event.  `produced`: what the kernels of phase 5 returned; their failure is waited for, and its time is not counted.
static fs3d_status update_end(fs3d_ctx *c, geom_clock t0, fs3d_status produced, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                              int n_seg_out[3], const char *name, bool slab)
{
    fs3d_status st = produced;
    if (st == FS3D_OK) st = BY_PREC(c, update_nodes_impl, c, type, bc_vel, bc_temp, name, slab, n_seg_out);
    hipStreamSynchronize(c->stream);                      // (a failure half way: the caller's arrays are not read after the call returns)
    gev_collect(c);
    if (produced) return produced;
    if (st == FS3D_OK) { c->have_nodes = true; c->n_create_segments++; }
    c->t_create_segments_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

// Every fs3d_update_nodes* entry, phase by phase.  `name` is the entry's, `slab` whether it takes an x-slab (a whole-grid context
// is the slab x_offset = 0, dimx = dimx_global); the source supplies its NULL test, its check and its producer.
// 1. the refusals; 2. the host clock of CreateSegments starts and the device is selected; 3. check(): everything that refuses
// the source (extrude_check, mesh_check) -- refused up to here, the context keeps the geometry it has and nothing is counted;
// 4. update_begin; 5. produce(a): the three byte arrays and the four value fields onto the device, a = geom_own_arrays (a source
// whose byte arrays are on the device already points a's at them); 6. update_end.
template <typename Check, typename Produce>
static fs3d_status update_run(fs3d_ctx *c, const char *name, bool slab, bool any_null, bool need_stage, Check check, Produce produce, int n_seg_out[3])
{
    GTRY(geom_refuse(c, name, any_null, slab ? nullptr : "moving geometry is"));
    if (!c->uploaded_once)
        return fail(c, FS3D_ERR_INVALID, std::string(name) + ": the first geometry comes through fs3d_upload_nodes; upload nodes first");
    const geom_clock t0 = std::chrono::steady_clock::now();
    HIPCHK(c, hipSetDevice(c->device));
    GTRY(check());
    // FS3D_OPT_FRESH_CELLS, a single context or (FS3D_OPT_FRESH_CELLS_SLABS) a slab of a group: the types of the geometry about to be
    // replaced, of the context's own planes (from here on the tables are rewritten)
    bool snapshot = false;
    if (c->opt_fresh_cells && (!geom_is_slab(c) || fresh_collective(c))) GTRY(fresh_snapshot(c, &snapshot));
    GTRY(update_begin(c, need_stage));
    NodeArrays a = geom_own_arrays(c);
    const fs3d_status st = produce(a);
    const fs3d_status done = update_end(c, t0, st, a.type, a.bc_vel, a.bc_temp, n_seg_out, name, slab);
    c->geom.prev_valid = snapshot && done == FS3D_OK;
    return done;
}

// Source 1, the node arrays of the global grid (a single context: its own), on the host or (dev) on the context's device.
struct ArraysIn { const uint8_t *b[3]; const void *v[4]; bool dev; };

static fs3d_status update_arrays(fs3d_ctx *c, const char *name, bool slab, const ArraysIn &in, int n_seg_out[3])
{
    const bool any_null = !in.b[0] || !in.b[1] || !in.b[2] || !in.v[0] || !in.v[1] || !in.v[2] || !in.v[3];
    return update_run(c, name, slab, any_null, !in.dev, [] { return FS3D_OK; }, [&](NodeArrays &a) -> fs3d_status {
        const size_t first = (size_t)c->x_offset * c->plane;
        uint8_t **own[3] = {&a.type, &a.bc_vel, &a.bc_temp};
        for (int q = 0; q < 3; q++) {
            if (in.dev) *own[q] = const_cast<uint8_t *>(in.b[q]);      // read where they are, never written
            else HIPCHK(c, hipMemcpyAsync(*own[q], in.b[q], (size_t)geom_gcell(c), hipMemcpyHostToDevice, c->stream));
        }
        // the four node-value fields are one of the tables: the context's planes, copied straight into place
        for (int v = 0; v < 4; v++) {
            const void *src = (const char *)in.v[v] + first * c->esize;
            if (a.v[v] != src) HIPCHK(c, hipMemcpyAsync(a.v[v], src, (size_t)c->ncell * c->esize, in.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        }
        return FS3D_OK;
    }, n_seg_out);
}

// Source 2, a Shape2D grid: on a slab the global one, given to every rank
static fs3d_status update_shape2d(fs3d_ctx *c, const char *name, bool slab, ExtrudeIn in, int n_seg_out[3])
{
    return update_run(c, name, slab, in.any_null(), true, [&] { return extrude_check(c, in, name); },
                      [&](NodeArrays &a) { return BY_PREC(c, extrude_launch, c, in, a, slab); }, n_seg_out);
}

// Source 3, a Shape3D mesh, with or without velocities.  On a slab every rank voxelises and fills the GLOBAL grid in its own staging
// buffer (mesh_launch), then builds the tables of its own planes.
static fs3d_status update_mesh(fs3d_ctx *c, const char *name, bool slab, const MeshIn &in, int n_seg_out[3])
{
    bool new_idx = false;
    return update_run(c, name, slab, in.any_null(), true, [&] { return mesh_check(c, in, name, &new_idx); },
                      [&](NodeArrays &a) { return BY_PREC(c, mesh_launch, c, in, new_idx, name, a); }, n_seg_out);
}

// The entries.  The slab ones: every rank is given the global input and
// rebuilds the tables of its own planes on its own stream; no rank talks to another one.
extern "C" fs3d_status fs3d_update_nodes(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                         const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    return update_arrays(c, "fs3d_update_nodes", false, {{type, bc_vel, bc_temp}, {vx, vy, vz, T}, false}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_slab(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                              const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    return update_arrays(c, "fs3d_update_nodes_slab", true, {{type, bc_vel, bc_temp}, {vx, vy, vz, T}, false}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_dev(fs3d_ctx *c, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                             const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3])
{
    return update_arrays(c, "fs3d_update_nodes_dev", false, {{type, bc_vel, bc_temp}, {vx, vy, vz, T}, true}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape2d(fs3d_ctx *c, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                                 double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{
    return update_shape2d(c, "fs3d_update_nodes_shape2d", false, {cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape2d_slab(fs3d_ctx *c, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                                      double dz, double depth, double depth_var, double baseT, int n_seg_out[3])
{
    return update_shape2d(c, "fs3d_update_nodes_shape2d_slab", true, {cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape3d(fs3d_ctx *c, const float *x, const float *y, const float *z, int nvert, const int *tri, int ntri,
                                                 double baseT, int n_seg_out[3])
{
    return update_mesh(c, "fs3d_update_nodes_shape3d", false, {x, y, z, nvert, tri, ntri, baseT}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape3d_slab(fs3d_ctx *c, const float *x, const float *y, const float *z, int nvert, const int *tri,
                                                      int ntri, double baseT, int n_seg_out[3])
{
    return update_mesh(c, "fs3d_update_nodes_shape3d_slab", true, {x, y, z, nvert, tri, ntri, baseT}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape3d_vel(fs3d_ctx *c, const float *x, const float *y, const float *z, const float *wx, const float *wy,
                                                     const float *wz, int nvert, const int *tri, int ntri, double baseT, double wallT, int n_seg_out[3])
{
    return update_mesh(c, "fs3d_update_nodes_shape3d_vel", false, {x, y, z, nvert, tri, ntri, baseT, true, wx, wy, wz, wallT}, n_seg_out);
}

extern "C" fs3d_status fs3d_update_nodes_shape3d_vel_slab(fs3d_ctx *c, const float *x, const float *y, const float *z, const float *wx,
                                                          const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                                          double wallT, int n_seg_out[3])
{
    return update_mesh(c, "fs3d_update_nodes_shape3d_vel_slab", true, {x, y, z, nvert, tri, ntri, baseT, true, wx, wy, wz, wallT}, n_seg_out);
}

// ---- the test aids: one stage of an update into the caller's device arrays; the context's geometry is not touched ----------------
extern "C" fs3d_status fs3d_extrude_shape2d_dev(fs3d_ctx *c, const uint8_t *cell2d, const float *velx2d, const float *vely2d, const float *T2d,
                                                double dz, double depth, double depth_var, double baseT, uint8_t *type_out,
                                                uint8_t *bc_vel_out, uint8_t *bc_temp_out, void *vx_out, void *vy_out, void *vz_out, void *T_out)
{
    const char *name = "fs3d_extrude_shape2d_dev";
    const NodeArrays out = {type_out, bc_vel_out, bc_temp_out, {vx_out, vy_out, vz_out, T_out}};
    ExtrudeIn in = {cell2d, velx2d, vely2d, T2d, dz, depth, depth_var, baseT};
    GTRY(geom_refuse(c, name, in.any_null() || out.any_null(), "the extrusion is"));
    GTRY(extrude_check(c, in, name));
    GTRY(BY_PREC(c, extrude_launch, c, in, out, false));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

static fs3d_status voxelize_dev(fs3d_ctx *c, const char *name, const MeshIn &in, const NodeArrays &out)
{
    GTRY(geom_refuse(c, name, in.any_null() || out.any_null(), "the voxelisation is"));
    bool new_idx = false;
    GTRY(mesh_check(c, in, name, &new_idx));
    gev_reset(c);                                        // (no update: its device time is not reported)
    const fs3d_status st = BY_PREC(c, mesh_launch, c, in, new_idx, name, out);
    const hipError_t e = hipStreamSynchronize(c->stream);
    gev_reset(c);
    if (st) return st;
    HIPCHK(c, e);
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_voxelize_shape3d_dev(fs3d_ctx *c, const float *x, const float *y, const float *z, int nvert, const int *tri, int ntri,
                                                 double baseT, uint8_t *type_out, uint8_t *bc_vel_out, uint8_t *bc_temp_out, void *vx_out,
                                                 void *vy_out, void *vz_out, void *T_out)
{
    return voxelize_dev(c, "fs3d_voxelize_shape3d_dev", {x, y, z, nvert, tri, ntri, baseT},
                        {type_out, bc_vel_out, bc_temp_out, {vx_out, vy_out, vz_out, T_out}});
}

extern "C" fs3d_status fs3d_voxelize_shape3d_vel_dev(fs3d_ctx *c, const float *x, const float *y, const float *z, const float *wx, const float *wy,
                                                     const float *wz, int nvert, const int *tri, int ntri, double baseT, double wallT,
                                                     uint8_t *type_out, uint8_t *bc_vel_out, uint8_t *bc_temp_out, void *vx_out, void *vy_out,
                                                     void *vz_out, void *T_out)
{
    return voxelize_dev(c, "fs3d_voxelize_shape3d_vel_dev", {x, y, z, nvert, tri, ntri, baseT, true, wx, wy, wz, wallT},
                        {type_out, bc_vel_out, bc_temp_out, {vx_out, vy_out, vz_out, T_out}});
}

// slab_what: as geom_refuse takes it
static fs3d_status flood_fill_dev(fs3d_ctx *c, const char *name, uint8_t *type_inout, const char *slab_what)
{
    GTRY(geom_refuse(c, name, !type_inout, slab_what));
    GTRY(mesh_prepare(c, 0, 0));
    gev_reset(c);
    const fs3d_status st = mesh_fill(c, type_inout, false, name);
    gev_reset(c);
    return st;
}

extern "C" fs3d_status fs3d_flood_fill_dev(fs3d_ctx *c, uint8_t *type_inout) { return flood_fill_dev(c, "fs3d_flood_fill_dev", type_inout, "the flood fill is"); }

// the same on the type array of the global grid, from any context (a slab: the fill does not stop at its cuts)
extern "C" fs3d_status fs3d_flood_fill_global_dev(fs3d_ctx *c, uint8_t *type_inout) { return flood_fill_dev(c, "fs3d_flood_fill_global_dev", type_inout, nullptr); }

extern "C" fs3d_status fs3d_mesh_fill_rounds(fs3d_ctx *c, int *rounds_out)
{
    if (!c || !rounds_out) return FS3D_ERR_INVALID;
    *rounds_out = c->geom.mesh_fill_rounds;
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_last_update_device_ms(fs3d_ctx *c, float *ms_out)
{
    if (!c || !ms_out) return FS3D_ERR_INVALID;
    *ms_out = c->geom.last_dev_ms;
    return FS3D_OK;
}

// ---- fresh cells --------------------------------------------------------------------------------------------------------------
// The fill of one layer from the previous types `prev` (device), on the context's stream; returns synchronised.  Batches of the
// device time as in mesh_fill: the classify pass up to the look at its count, then FRESH_BATCH rounds per look at their counters.
// One body: a single context is the group of one rank that exchanges nothing and sums nothing.  `coll`, a slab of a group
// (fresh_collective): the tag array has a ghost plane on either side, as the fields have; before every round one grouped exchange
// (fs3d_comm_fill_exchange) brings the neighbours' boundary planes of the four fields and of the tags as the round before left them;
// the count of fresh cells and, per batch, the counts of its rounds are summed over the ranks (fs3d_comm_allreduce_sum2), so every
// rank sees the same numbers, ends in the same round and makes the same exchanges and sums whatever it holds.  Every wait is the
// transport's.  The device time is that of the rank's own kernels and copies; the transport's copies and waits are not in it.
template <typename R>
static fs3d_status fresh_fill_impl(fs3d_ctx *c, const uint8_t *prev, int layer, int max_rounds, bool coll, long long info[4])
{
    fs3d_geom &g = c->geom;
    const long long ncell = c->ncell;
    long long *const na = &c->geom_allocs;
    // a slab of a group: [pad][ghost plane][owned planes][ghost plane], the first owned cell aligned to 8 bytes (k_fresh_classify<8>)
    g.fill_tag_off = coll ? (c->plane + 7) / 8 * 8 : 0;
    BUFCHK(c, g.fill_tag.reserve((size_t)(g.fill_tag_off + ncell + (coll ? c->plane : 0)), na));
    BUFCHK(c, g.fill_cnt.reserve(FC_WORDS * sizeof(unsigned), na));
    BUFCHK(c, g.fill_host.reserve(FC_WORDS * sizeof(unsigned)));
    if (coll) BUFCHK(c, g.fill_red.reserve(2 * sizeof(double), na));
    if (coll) BUFCHK(c, g.fill_red_host.reserve(2 * sizeof(double)));
    if (!g.fill_list) {                                     // the fresh cells are a thin shell: an eighth of the grid to begin with
        const long long cap = std::min<long long>(ncell, ncell / 8 + 1024);
        BUFCHK(c, g.fill_list.replace(sizeof(int) * (size_t)cap, na));
        g.fill_cap = cap;
    }
    uint8_t *tag = g.fill_tag + g.fill_tag_off;            // the first owned cell's
    const int buf = c->slot[layer];
    R *f[4];
    for (int v = 0; v < 4; v++) f[v] = (R *)((char *)c->lay[buf] + ((size_t)v * c->fstride + c->plane) * c->esize);
    const bool vec = ((uintptr_t)prev & 7) == 0;
    long long fresh = 0;
    for (;;) {
        gev_begin(c);
        HIPCHK(c, hipMemsetAsync(g.fill_cnt, 0, FC_WORDS * sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(vec ? k_fresh_classify<8> : k_fresh_classify<1>, dim3(grid_for(vec ? (ncell + 7) / 8 : ncell)), dim3(256), 0, c->stream,
                           c->code, prev, ncell, tag, g.fill_list, g.fill_cap, g.fill_cnt);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(g.fill_host, g.fill_cnt, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        GTRY(gev_sync(c));
        fresh = (long long)g.fill_host[FC_FRESH];
        if (fresh <= g.fill_cap) break;
        g.fill_cap = 0;                                     // grow-only, with headroom: the shell of a moving wall breathes
        const long long cap = std::min<long long>(ncell, fresh + fresh / 4 + 1024);
        BUFCHK(c, g.fill_list.replace(sizeof(int) * (size_t)cap, na));
        g.fill_cap = cap;
    }
    // the collective fill: the counter words [at, at + n), n <= 2, summed over the ranks into fill_red_host; returns synchronised
    auto sum_counts = [&](int at, int n) -> fs3d_status {
        gev_begin(c);
        hipLaunchKernelGGL(k_fresh_counts, dim3(1), dim3(64), 0, c->stream, g.fill_cnt + at, n, g.fill_red);
        HIPCHK(c, hipGetLastError());
        gev_end(c);
        GTRY(fs3d_comm_allreduce_sum2(c, g.fill_red));
        HIPCHK(c, hipMemcpyAsync(g.fill_red_host, g.fill_red, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FS3D_OK;
    };
    long long all_fresh = fresh;                            // over the ranks
    if (coll) { GTRY(sum_counts(FC_FRESH, 1)); all_fresh = (long long)g.fill_red_host[0]; }
    const auto round_kernel = coll ? k_fresh_round<R, true> : k_fresh_round<R, false>;
    const int lo = coll && c->rank > 0, hi = coll && c->rank + 1 < c->nranks;
    const int limit = max_rounds ? max_rounds : FRESH_MAX_ROUNDS;
    long long filled = 0, all_filled = 0;
    int rounds = 0;
    bool done = all_fresh == 0;
    for (int r = 1; !done && r <= limit; r += FRESH_BATCH) {
        const int nb = std::min(FRESH_BATCH, limit - r + 1);
        for (int q = 0; q < nb; q++) {
            if (coll) { gev_end(c); GTRY(fs3d_comm_fill_exchange(c, buf, tag)); }      // the state after round r + q - 1
            gev_begin(c);
            hipLaunchKernelGGL(round_kernel, dim3(grid_for(fresh, 1 << 30)), dim3(256), 0, c->stream,
                               g.fill_list, fresh, tag, r + q, c->dimx, c->dimy, c->dimz, f[0], f[1], f[2], f[3], g.fill_cnt + r + q, lo, hi);
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(g.fill_host + r, g.fill_cnt + r, nb * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        if (coll) { gev_end(c); GTRY(sum_counts(r, nb)); } else GTRY(gev_sync(c));
        for (int q = 0; q < nb && !done; q++) {             // a round that fills nothing ends the fill; so does the last fresh cell
            const long long n = (long long)g.fill_host[r + q], all_n = coll ? (long long)g.fill_red_host[q] : n;
            if (!all_n) { done = true; break; }
            rounds++; filled += n; all_filled += all_n;
            done = all_filled == all_fresh;
        }
    }
    info[0] = fresh; info[1] = filled; info[2] = rounds; info[3] = fresh - filled;
    return FS3D_OK;
}

// own: the plain entry, which reads the snapshot the context keeps; else `prev` is the caller's
static fs3d_status fresh_fill(fs3d_ctx *c, const char *name, bool own, const uint8_t *prev, int layer, int max_rounds, long long info[4])
{
    GTRY(geom_refuse(c, name, (!own && !prev) || !info, nullptr));
    const bool coll = fresh_collective(c);
    if (geom_is_slab(c) && !coll) {
        if (c->opt_fresh_slabs)
            return fail(c, FS3D_ERR_UNSUPPORTED, std::string(name) + ": FS3D_OPT_FRESH_CELLS_SLABS: a lone x-slab of a larger grid needs its neighbours' "
                         "planes: make it a member of a group (fs3d_comm_init_local, fs3d_comm_init) first");
        return geom_refuse(c, name, false, "the fresh-cell fill is");
    }
    if (layer < 0 || layer > 3) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": bad layer id");
    if (max_rounds < 0 || max_rounds > FRESH_MAX_ROUNDS) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": max_rounds is 0 .. 250 (0: 250)");
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": upload nodes first");
    if (own) {
        if (!c->opt_fresh_cells) return fail(c, FS3D_ERR_INVALID, std::string(name) + ": FS3D_OPT_FRESH_CELLS is off: no update keeps the previous node types");
        if (!c->geom.prev_valid || !c->geom.prev_type)
            return fail(c, FS3D_ERR_INVALID, std::string(name) + ": no previous geometry: no fs3d_update_nodes* has succeeded (with FS3D_OPT_FRESH_CELLS on, "
                         "on a context that had a geometry) since the last fs3d_upload_nodes");
        prev = c->geom.prev_type;
    }
    // the tag array of a slab has ghost planes, a single context's has none: one that was allocated in the other form is refused
    if (c->geom.fill_tag && (c->geom.fill_tag_off != 0) != coll)
        return fail(c, FS3D_ERR_INVALID, std::string(name) + ": the context has filled fresh cells before it joined its group; join the group before the first fill");
    HIPCHK(c, hipSetDevice(c->device));
    gev_reset(c);
    const fs3d_status st = BY_PREC(c, fresh_fill_impl, c, prev, layer, max_rounds, coll, info);
    if (st) {                                               // a rank that fails takes the group down: its peers return FS3D_ERR_COMM
        if (coll) fs3d_comm_abort(c);
        hipStreamSynchronize(c->stream); gev_reset(c);
        return st;
    }
    c->geom.last_fill_ms = gev_take(c) + (own ? c->geom.snap_ms : 0.0f);
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_fill_fresh_cells_dev(fs3d_ctx *c, const uint8_t *prev_type_dev, int layer, int max_rounds, long long info[4])
{
    return fresh_fill(c, "fs3d_fill_fresh_cells_dev", false, prev_type_dev, layer, max_rounds, info);
}

extern "C" fs3d_status fs3d_fill_fresh_cells(fs3d_ctx *c, int layer, int max_rounds, long long info[4])
{
    return fresh_fill(c, "fs3d_fill_fresh_cells", true, nullptr, layer, max_rounds, info);
}

extern "C" fs3d_status fs3d_last_fill_device_ms(fs3d_ctx *c, float *ms_out)
{
    if (!c || !ms_out) return FS3D_ERR_INVALID;
    *ms_out = c->geom.last_fill_ms;
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_geometry_dead_lines(fs3d_ctx *c, int dir, uint8_t *dead_out, long long *n_lines_out)
{
    if (!c) return FS3D_ERR_INVALID;
    if (dir < 0 || dir > 2) return fail(c, FS3D_ERR_INVALID, "fs3d_geometry_dead_lines: bad direction");
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_geometry_dead_lines: upload nodes first");
    const long long n = geom_lines(c, dir).nlines;
    if (n_lines_out) *n_lines_out = n;
    if (!dead_out) return FS3D_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dead_out, c->dead[dir], (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_clear_outer_cells(fs3d_ctx *c, int layer, double baseT)
{
    if (!c) return FS3D_ERR_INVALID;
    if (layer < 0 || layer > 3) return fail(c, FS3D_ERR_INVALID, "fs3d_clear_outer_cells: bad layer id");
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_clear_outer_cells: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    char *f[4];
    for (int v = 0; v < 4; v++) f[v] = (char *)c->lay[c->slot[layer]] + ((size_t)v * c->fstride + c->plane) * c->esize;
    if (c->prec == FS3D_F32)
        hipLaunchKernelGGL((k_clear_outer<float>), dim3(grid_for(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell, (float)baseT,
                           (float *)f[0], (float *)f[1], (float *)f[2], (float *)f[3]);
    else
        hipLaunchKernelGGL((k_clear_outer<double>), dim3(grid_for(c->ncell)), dim3(256), 0, c->stream, c->code, c->ncell, baseT,
                           (double *)f[0], (double *)f[1], (double *)f[2], (double *)f[3]);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FS3D_OK;
}

extern "C" fs3d_status fs3d_geometry_info(fs3d_ctx *c, long long info[FS3D_N_GEOM_INFO])
{
    if (!c || !info) return FS3D_ERR_INVALID;
    if (!c->have_nodes) return fail(c, FS3D_ERR_INVALID, "fs3d_geometry_info: upload nodes first");
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < FS3D_N_GEOM_INFO; k++) info[k] = 0;
    for (int d = 0; d < 3; d++) info[d] = c->nseg[d];
    info[3] = c->n_bnd;
    info[4] = c->stale_in_cells;
    std::vector<uint8_t> hb;
    for (int d = 0; d < 3; d++) {
        hb.resize((size_t)geom_lines(c, d).nlines);
        HIPCHK(c, hipMemcpyAsync(hb.data(), c->dead[d], hb.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint8_t b : hb) info[5 + d] += b != 0;
    }
    for (int d = 0; d < 2; d++) {
        if (!c->uflag[d]) continue;
        std::vector<unsigned> fl((size_t)geom_lines(c, d).n_o * geom_ng(c));
        HIPCHK(c, hipMemcpyAsync(fl.data(), c->uflag[d], fl.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (unsigned f : fl) info[8 + d] += f & 1;
        info[10 + d] = c->n_ucol[d];
    }
    // the digest comes from the table the sweeps read; its device word is borrowed from the EvalDivError partials (rewritten by every evaluation)
    unsigned long long *dw = (unsigned long long *)c->red_buf, hw = 0;
    HIPCHK(c, hipMemsetAsync(dw, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_geom_digest, dim3(grid_for(c->ncell, 1024)), dim3(256), 0, c->stream, c->code, c->ncell, dw);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&hw, dw, sizeof hw, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    info[12] = (long long)hw;
    info[13] = c->geom_allocs;
    return FS3D_OK;
}
