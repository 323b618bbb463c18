// Stand-alone check of the shared voxel rule (cmc_fluid_solver_amd/csrc/fs3d_voxel.h) without the loader: the arithmetic the kernels
// run, on a CPU, built with the address and undefined-behaviour sanitizers by tests/test_voxel_rule.py:
//   voxel_rule_test <in> <out> <shell>
//   in:  int32 dimx, dimy, dimz, nvert, ntri; float32 x, y, z, wx, wy, wz [nvert each] (grid coordinates, velocities); int32 tri[3 * ntri]
//   out: uint8 wall[dimx * dimy * dimz] (1 where a triangle sets the cell; no fill), int32 owner[..] (-1 off the walls),
//        float64 ux[..], uy[..], uz[..] (the wall velocity of the cell's owner, 0 off the walls)
//   shell: 0 the conservative shell, 1 the thin one
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmc_fluid_solver_amd/csrc/fs3d_voxel.h"

struct Mesh {
    int dimx, dimy, dimz;
    std::vector<float> a[6];              // x, y, z, wx, wy, wz
    std::vector<int32_t> tri;
};

template <bool THIN>
static void voxelise(const Mesh &m, std::vector<uint8_t> &wall, std::vector<int32_t> &owner)
{
    for (size_t t = 0; 3 * t < m.tri.size(); t++) {
        float p[3][3];
        for (int v = 0; v < 3; v++)
            for (int c = 0; c < 3; c++) p[v][c] = m.a[c][m.tri[3 * t + v]];
        VoxelSetup s;
        if (!voxel_setup<THIN>(p, m.dimx, m.dimy, m.dimz, s)) continue;
        const size_t plane = (size_t)m.dimy * m.dimz;
        const size_t sa = voxel_sel(s.a, plane, (size_t)m.dimz, (size_t)1), sb = voxel_sel(s.b, plane, (size_t)m.dimz, (size_t)1),
                     sd = voxel_sel(s.d, plane, (size_t)m.dimz, (size_t)1);
        const size_t base = ((size_t)s.o[0] * m.dimy + s.o[1]) * m.dimz + s.o[2];
        for (int ia = 0; ia < s.cnt[0]; ia++)
            for (int ib = 0; ib < s.cnt[1]; ib++) {
                VoxelColumn c;
                if (!voxel_column<THIN>(s, ia, ib, c)) continue;
                for (int k = c.k0; k <= c.k1; k++) {
                    if (!voxel_cell<THIN>(s, c, k)) continue;
                    const size_t cell = base + ia * sa + ib * sb + k * sd;
                    wall.at(cell) = 1;
                    if (owner[cell] < 0) owner[cell] = (int32_t)t;          // triangles come in ascending order
                }
            }
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: %s <in> <out> <shell>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t head[5];
    if (std::fread(head, sizeof head, 1, f) != 1) return 2;
    Mesh m{head[0], head[1], head[2], {}, {}};
    const size_t nvert = (size_t)head[3], ntri = (size_t)head[4];
    bool ok = true;
    for (auto &a : m.a) { a.resize(nvert); ok = ok && (nvert == 0 || std::fread(a.data(), 4, nvert, f) == nvert); }
    m.tri.resize(3 * ntri);
    ok = ok && (ntri == 0 || std::fread(m.tri.data(), 4, 3 * ntri, f) == 3 * ntri);
    std::fclose(f);
    for (int32_t v : m.tri) ok = ok && v >= 0 && (size_t)v < nvert;
    if (!ok) { std::fprintf(stderr, "short or bad input\n"); return 2; }
    const size_t ncell = (size_t)m.dimx * m.dimy * m.dimz;
    std::vector<uint8_t> wall(ncell, 0);
    std::vector<int32_t> owner(ncell, -1);
    if (std::atoi(argv[3])) voxelise<true>(m, wall, owner); else voxelise<false>(m, wall, owner);
    std::vector<double> u[3];
    for (auto &a : u) a.assign(ncell, 0.0);
    for (size_t cell = 0; cell < ncell; cell++) {
        if (owner[cell] < 0) continue;
        const int k = (int)(cell % m.dimz), j = (int)((cell / m.dimz) % m.dimy), i = (int)(cell / ((size_t)m.dimz * m.dimy));
        D3 q[3], W[3];
        for (int v = 0; v < 3; v++) {
            const int iv = m.tri[3 * (size_t)owner[cell] + v];
            q[v] = {(double)m.a[0][iv] - (double)i, (double)m.a[1][iv] - (double)j, (double)m.a[2][iv] - (double)k};
            W[v] = {(double)m.a[3][iv], (double)m.a[4][iv], (double)m.a[5][iv]};
        }
        const D3 r = wall_velocity(q[0], q[1], q[2], W[0], W[1], W[2]);
        u[0][cell] = r.x; u[1][cell] = r.y; u[2][cell] = r.z;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    std::fwrite(wall.data(), 1, ncell, f);
    std::fwrite(owner.data(), 4, ncell, f);
    for (auto &a : u) std::fwrite(a.data(), 8, ncell, f);
    std::fclose(f);
    return 0;
}
