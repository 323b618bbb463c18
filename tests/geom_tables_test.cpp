// The host definition of the geometry tables (cmc_fluid_solver_amd/csrc/fs3d_tables.h) on a CPU, no GPU library:
//     geom_tables_test IN OUT
// IN:  five int32 (gx, dimy, dimz, x0, nx), then type, bc_vel, bc_temp of the GLOBAL grid, gx * dimy * dimz bytes each.
// OUT: every field of GeomTables.  20 int64 -- nseg[3], stale_in_cells, shared_free, has_columns[2], n_ucol[2], then the
//      element counts of code, dead[3], ucol[2], uflag[2], bnd_idx, and two spare zeros -- followed by those arrays in that order.
// tests/test_geom_tables.py builds it with the address and undefined-behaviour sanitizers and compares with a numpy restatement.
#include <cstdio>
#include <vector>

#include "../cmc_fluid_solver_amd/csrc/fs3d_tables.h"

template <typename T> static bool put(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int32_t h[5];
    if (fread(h, sizeof h[0], 5, in) != 5) { fprintf(stderr, "%s: short header\n", argv[1]); return 2; }
    const int gx = h[0], dimy = h[1], dimz = h[2], x0 = h[3], nx = h[4];
    if (gx < 1 || dimy < 1 || dimz < 1 || x0 < 0 || nx < 1 || x0 + nx > gx) { fprintf(stderr, "%s: bad dimensions\n", argv[1]); return 2; }
    const size_t n = (size_t)gx * dimy * dimz;
    std::vector<uint8_t> a[3];
    for (auto &v : a) {
        v.resize(n);
        if (fread(v.data(), 1, n, in) != n) { fprintf(stderr, "%s: short array\n", argv[1]); return 2; }
    }
    fclose(in);

    const GeomTables t = build_geom_tables(gx, dimy, dimz, x0, nx, a[0].data(), a[1].data(), a[2].data());

    const long long head[20] = {t.nseg[0], t.nseg[1], t.nseg[2], t.stale_in_cells, t.shared_free, t.has_columns[0], t.has_columns[1],
                                t.n_ucol[0], t.n_ucol[1], (long long)t.code.size(), (long long)t.dead[0].size(),
                                (long long)t.dead[1].size(), (long long)t.dead[2].size(), (long long)t.ucol[0].size(),
                                (long long)t.ucol[1].size(), (long long)t.uflag[0].size(), (long long)t.uflag[1].size(),
                                (long long)t.bnd_idx.size(), 0, 0};
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    bool ok = fwrite(head, sizeof head[0], 20, out) == 20 && put(out, t.code);
    for (int d = 0; d < 3; d++) ok = ok && put(out, t.dead[d]);
    for (int d = 0; d < 2; d++) ok = ok && put(out, t.ucol[d]);
    for (int d = 0; d < 2; d++) ok = ok && put(out, t.uflag[d]);
    ok = ok && put(out, t.bnd_idx);
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "%s: write failed\n", argv[2]); return 2; }
    return 0;
}
