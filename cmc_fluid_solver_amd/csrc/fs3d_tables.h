// The geometry tables of one context -- cell codes, dead lines, shared code columns, the BOUND / VALVE list -- from the node arrays.
// Host only: no HIP header, any C++17 compiler will do (tests/geom_tables_test.cpp runs it on a CPU).  The definition of every table:
// fs3d_upload_nodes (fs3d_hip.hip) writes what build_geom_tables returns; the device builder (kernels_geom.hip) is held to it bit for bit.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/fs3d.h"

// ---- per-cell code word (uint16) ------------------------------------------------
// bits 0..3   row code of the X sweep
// bits 4..7   row code of the Y sweep
// bits 8..11  row code of the Z sweep
// bits 12..13 NodeType (Geometry.h:31-36)
// row code: bits 0..1 kind, bit 2 velocity BC is FREE, bit 3 temperature BC is FREE
// (BC bits are only meaningful for START/END rows).
// The kinds restate Grid3D::GenerateListSegments (Grid3D.cpp:47-127) per cell: a
// segment is START, INTERIOR.., END along its line; everything else is SKIP.
enum { ROW_SKIP = 0, ROW_INTERIOR = 1, ROW_START = 2, ROW_END = 3 };
#define ROW_VELFREE 4
#define ROW_TEMPFREE 8
#define CODE_TYPE_SHIFT 12
#define UCOL_PITCH 512                 // codes per shared column (the partition kernels take lines of <= 512 cells)

// The tables of the planes [x0, x0 + nx) of a grid of gx x dimy x dimz cells.  Local index l = (i - x0) * dimy * dimz + j * dimz + k;
// lines of X: [j][k], of Y: [i - x0][k], of Z: [i - x0][j].
struct GeomTables {
    std::vector<uint16_t> code;            // per local cell, bits as above
    long long nseg[3] = {0, 0, 0};         // segments per direction; X lines span all slabs: nseg[0] counts the global segments
    bool shared_free = false;              // a FREE cell closes one segment and opens the next: refused, no table below is built
    std::vector<uint8_t> dead[3];          // per line: 1 = no cell of the local line is on a segment of that direction or NODE_IN
    long long stale_in_cells = 0;          // NODE_IN cells on no segment, summed over the directions
    bool has_columns[2] = {false, false};  // X, Y: false where the local lines are longer than UCOL_PITCH (then nothing below)
    std::vector<uint16_t> ucol[2];         // n_ucol distinct columns of UCOL_PITCH codes (one zero column when there is none)
    std::vector<unsigned> uflag[2];        // [o][group]: bit 0 uniform, bit 1 the pair is, bits 2.. the column id
    int n_ucol[2] = {0, 0};
    std::vector<int> bnd_idx;              // local indices of the NODE_BOUND / NODE_VALVE cells, ascending
};

// Per-line restatement of Grid3D::GenerateListSegments (Grid3D.cpp:47-127, nblockZ = 1):
// walk the line; a run of NODE_IN cells opened at pos+1 takes the cell at pos as its
// first node and the first non-IN cell after it as its last node; a run that reaches the
// end of the line without a closing cell is dropped.  kinds[] gets START/INTERIOR/END.
// Returns the number of segments; *shared_free is set when a cell closes one segment and
// opens the next while carrying a FREE boundary condition (two different rows on one cell).
static int line_kinds(const uint8_t *type, long long base, long long stride, int n, uint8_t *kinds,
                      const uint8_t *bc_vel, const uint8_t *bc_temp, bool *shared_free)
{
    int nseg = 0, state = 0, start = 0;
    for (int s = 0; s < n; s++) kinds[s] = ROW_SKIP;
    for (int pos = 0; pos + 1 < n; pos++) {
        if (type[base + (long long)(pos + 1) * stride] == FS3D_NODE_IN) {
            if (state == 0) start = pos;
            state = 1;
        } else if (state == 1) {
            const int end = pos + 1;
            if (kinds[start] == ROW_END) {   // closes the previous segment and opens this one
                const long long id = base + (long long)start * stride;
                if (bc_vel[id] == FS3D_BC_FREE || bc_temp[id] == FS3D_BC_FREE) *shared_free = true;
            }
            kinds[start] = ROW_START;
            for (int s = start + 1; s < end; s++) kinds[s] = ROW_INTERIOR;
            kinds[end] = ROW_END;
            nseg++;
            state = 0;
        }
    }
    return nseg;
}

// Cell codes of the local planes, with nseg and shared_free: the node type of every cell, and per direction the row kind from the
// walk of the cell's line plus, on START and END cells, the FREE bits of its boundary conditions.
static void geom_cell_codes(int gx, int dimy, int dimz, int x0, int nx, const uint8_t *type, const uint8_t *bc_vel,
                            const uint8_t *bc_temp, GeomTables &t)
{
    const long long plane = (long long)dimy * dimz, first = (long long)x0 * plane, ncell = plane * nx;
    t.code.resize((size_t)ncell);
    for (long long l = 0; l < ncell; l++) t.code[(size_t)l] = (uint16_t)((type[first + l] & 3) << CODE_TYPE_SHIFT);
    std::vector<uint8_t> kinds((size_t)std::max(gx, std::max(dimy, dimz)));
    // one line of direction d: its kinds from the walk; its cells [s0, s1) are local
    auto line = [&](int d, long long base, long long stride, int n, int s0, int s1) {
        t.nseg[d] += line_kinds(type, base, stride, n, kinds.data(), bc_vel, bc_temp, &t.shared_free);
        for (int s = s0; s < s1; s++) {
            const long long gid = base + s * stride;
            const bool ends = kinds[s] == ROW_START || kinds[s] == ROW_END;
            const int rc = kinds[s] | (ends && bc_vel[gid] == FS3D_BC_FREE ? ROW_VELFREE : 0) | (ends && bc_temp[gid] == FS3D_BC_FREE ? ROW_TEMPFREE : 0);
            t.code[(size_t)(gid - first)] |= (uint16_t)(rc << (4 * d));
        }
    };
    // X lines span all slabs: kinds come from the global line (the reference clips global segments per device, AdiSolver3D.cpp:475-524)
    for (int j = 0; j < dimy; j++)
        for (int k = 0; k < dimz; k++) line(0, (long long)j * dimz + k, plane, gx, x0, x0 + nx);
    for (int i = x0; i < x0 + nx; i++) {
        for (int k = 0; k < dimz; k++) line(1, i * plane + k, dimz, dimy, 0, dimy);
        for (int j = 0; j < dimy; j++) line(2, i * plane + (long long)j * dimz, 1, dimz, 0, dimz);
    }
}

// Dead lines and stale_in_cells, from the codes.  Dead: no cell of the (local part of the) line is on a segment of that direction or NODE_IN -- nothing a sweep computes for such a
// line is ever stored; the partition kernels keep them off the row-kind paths.
// Stale: NODE_IN cells that lie on no segment of some direction (a run without a closing cell, Grid3D.cpp:87-117): the reference
// merges the STALE `next` value there -- whatever an earlier sweep left.  Only a geometry without such cells lets the time step drop
// stores of `next` that nothing but they could read (time_step_enqueue).
static void geom_dead_lines(int dimy, int dimz, int nx, GeomTables &t)
{
    const size_t nlines[3] = {(size_t)dimy * dimz, (size_t)nx * dimz, (size_t)nx * dimy};
    for (int d = 0; d < 3; d++) t.dead[d].assign(nlines[d], 1);
    const uint16_t *code = t.code.data();
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < dimy; j++)
            for (int k = 0; k < dimz; k++, code++) {
                const bool in = ((*code >> CODE_TYPE_SHIFT) & 3) == FS3D_NODE_IN;
                const size_t line[3] = {(size_t)j * dimz + k, (size_t)i * dimz + k, (size_t)i * dimy + j};
                for (int d = 0; d < 3; d++) {
                    const bool skip = ((*code >> (4 * d)) & 3) == ROW_SKIP;
                    if (in || !skip) t.dead[d][line[d]] = 0;
                    t.stale_in_cells += in && skip;
                }
            }
}

// Shared code columns of direction d (X, d = 0: o = j, the n = nx cells of a line along i; Y, d = 1: o = i, the n = dimy cells along
// j), from the codes and dead[d].  The dimz lines of one o fall into ng = ceil(dimz / 32) groups of 32 neighbouring k; the column of
// a line is its n codes masked to (row code of d, node type).  Where every live line of a group carries the same column, the
// partition kernels read that one column instead of 2 bytes per cell.  Three rules:
//   1. Group uniformity.  Bit 0 of a group's flag: all its live lines have equal columns (a group without a live line counts as
//      uniform).  Its column is that of its first live line, zeros when it has none.
//   2. The pair rule, on even g only (a 64-line tile reads the column of g for g and g + 1).  Bit 1: bit 0 is set, and either g is
//      the last group, or bit 0 of g + 1 is set and the two columns are equal on [0, n) or one of the two groups is all dead.  An
//      all-dead g whose partner is live takes the partner's column; an all-dead g + 1 keeps its zeros.
//   3. Numbering by first appearance.  The distinct columns of the uniform groups get the ids 0, 1, .. in the order in which
//      q = o * ng + g ascending first shows them (a box has two: its live lines', and zeros -- they stay in the caches);
//      uflag[q] = flag bits | id << 2, and 0 for a group that is not uniform.  ucol[id] is the column, zero from n to UCOL_PITCH;
//      without a uniform group n_ucol is 0 and ucol is one zero column.
static void geom_shared_columns(int d, int dimy, int dimz, int nx, GeomTables &t)
{
    const int n_o = d == 0 ? dimy : nx, n = d == 0 ? nx : dimy, ng = (dimz + 31) / 32;
    t.has_columns[d] = n <= UCOL_PITCH;
    if (!t.has_columns[d]) return;
    const uint16_t keep = (uint16_t)((0xF << (4 * d)) | (3 << CODE_TYPE_SHIFT));
    const long long plane = (long long)dimy * dimz, ss = d == 0 ? plane : dimz, os = d == 0 ? dimz : plane;
    const std::vector<uint8_t> &dead = t.dead[d];
    const size_t nq = (size_t)n_o * ng;
    std::vector<uint16_t> col(nq * UCOL_PITCH, 0);
    std::vector<uint8_t> flag(nq, 0), all_dead(nq, 0);
    // 1. group uniformity
    for (int o = 0; o < n_o; o++)
        for (int g = 0; g < ng; g++) {
            const size_t q = (size_t)o * ng + g;
            uint16_t *cc = &col[q * UCOL_PITCH];
            int k0 = -1;
            bool uni = true;
            for (int k = 32 * g; k < std::min(32 * g + 32, dimz) && uni; k++) {
                if (dead[(size_t)o * dimz + k]) continue;
                const uint16_t *src = &t.code[(size_t)((long long)o * os + k)];
                if (k0 < 0) { k0 = k; for (int s = 0; s < n; s++) cc[s] = (uint16_t)(src[(size_t)s * ss] & keep); }
                else for (int s = 0; s < n; s++) if ((uint16_t)(src[(size_t)s * ss] & keep) != cc[s]) { uni = false; break; }
            }
            flag[q] = uni ? 1 : 0; all_dead[q] = k0 < 0;
        }
    // 2. the pair rule
    for (int o = 0; o < n_o; o++)
        for (int g = 0; g < ng; g += 2) {
            const size_t q = (size_t)o * ng + g;
            bool pair = flag[q] & 1;
            if (pair && g + 1 < ng) {
                uint16_t *a = &col[q * UCOL_PITCH], *b = a + UCOL_PITCH;
                pair = flag[q + 1] & 1;
                if (pair && all_dead[q] && !all_dead[q + 1]) std::copy(b, b + UCOL_PITCH, a);
                else if (pair && !all_dead[q] && !all_dead[q + 1]) pair = std::equal(a, a + n, b);
            }
            if (pair) flag[q] |= 2;
        }
    // 3. numbering by first appearance
    std::map<std::string, unsigned> ids;
    t.uflag[d].assign(nq, 0);
    for (size_t q = 0; q < nq; q++) {
        if (!flag[q]) continue;
        const uint16_t *cc = &col[q * UCOL_PITCH];
        const std::string key((const char *)cc, (size_t)n * sizeof(uint16_t));
        auto it = ids.find(key);
        if (it == ids.end()) {
            it = ids.emplace(key, (unsigned)ids.size()).first;
            t.ucol[d].insert(t.ucol[d].end(), cc, cc + UCOL_PITCH);
        }
        t.uflag[d][q] = (unsigned)flag[q] | (it->second << 2);
    }
    t.n_ucol[d] = (int)ids.size();
    if (t.ucol[d].empty()) t.ucol[d].resize(UCOL_PITCH, 0);
}

// The tables of the planes [x0, x0 + nx) from the GLOBAL node arrays (gx * dimy * dimz entries each).
static GeomTables build_geom_tables(int gx, int dimy, int dimz, int x0, int nx, const uint8_t *type, const uint8_t *bc_vel,
                                    const uint8_t *bc_temp)
{
    GeomTables t;
    geom_cell_codes(gx, dimy, dimz, x0, nx, type, bc_vel, bc_temp, t);
    if (t.shared_free) return t;
    geom_dead_lines(dimy, dimz, nx, t);
    for (int d = 0; d < 2; d++) geom_shared_columns(d, dimy, dimz, nx, t);
    const uint8_t *local = type + (long long)x0 * dimy * dimz;
    for (size_t l = 0; l < t.code.size(); l++)
        if (local[l] == FS3D_NODE_BOUND || local[l] == FS3D_NODE_VALVE) t.bnd_idx.push_back((int)l);
    return t;
}
