// Stand-alone check of the conservative voxeliser of host/Shape3D.h (Shape3D::voxels = 1), built with the address and
// undefined-behaviour sanitizers by tests/test_mesh_watertight.py:  mesh_voxel_test <in> <out>
//   in:  int32 dimx, dimy, dimz, nvert, ntri; float32 x[nvert], y[nvert], z[nvert] (grid coordinates); int32 tri[3 * ntri]
//   out: the dimx * dimy * dimz node types after Build (voxeliser and flood fill)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../cmc_fluid_solver_amd/host/Shape3D.h"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t head[5];
    if (std::fread(head, sizeof head, 1, f) != 1) return 2;
    const int nvert = head[3], ntri = head[4];
    fs3d::Shape3DFrame fr;
    fr.x.resize(nvert); fr.y.resize(nvert); fr.z.resize(nvert); fr.idx.resize(3 * (size_t)ntri);
    bool ok = true;
    for (std::vector<float> *a : {&fr.x, &fr.y, &fr.z}) ok = ok && (nvert == 0 || std::fread(a->data(), 4, nvert, f) == (size_t)nvert);
    ok = ok && (ntri == 0 || std::fread(fr.idx.data(), 4, 3 * (size_t)ntri, f) == 3 * (size_t)ntri);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
    fs3d::Shape3D sh;
    sh.dimx = head[0]; sh.dimy = head[1]; sh.dimz = head[2];
    sh.voxels = 1;
    try { sh.BuildMesh(fr); }
    catch (const std::exception &e) { std::fprintf(stderr, "refused: %s\n", e.what()); return 3; }
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    std::fwrite(sh.type.data(), 1, sh.type.size(), f);
    std::fclose(f);
    return 0;
}
