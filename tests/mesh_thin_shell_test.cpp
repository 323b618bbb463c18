// Stand-alone check of the thin shell of host/Shape3D.h (Shape3D::voxels = 1, Shape3D::shell = 1), built with the address and
// undefined-behaviour sanitizers by tests/test_mesh_thin_shell.py:  mesh_thin_shell_test <in> <out> <voxels> <shell>
//   in:  int32 dimx, dimy, dimz, nvert, ntri; float32 x[nvert], y[nvert], z[nvert] (grid coordinates); int32 tri[3 * ntri]
//   out: the dimx * dimy * dimz node types after Build (voxeliser and flood fill), then -- with voxels = 1 -- the int32 owner of
//        every cell (the mesh is built with vertex velocities, all zero, so that the owners are kept)
// Exit status 3: Build refused the mesh or the modes (the message on stderr).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cmc_fluid_solver_amd/host/Shape3D.h"

int main(int argc, char **argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: %s <in> <out> <voxels> <shell>\n", argv[0]); return 2; }
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
    sh.voxels = std::atoi(argv[3]);
    sh.shell = std::atoi(argv[4]);
    if (sh.voxels == 1) {
        sh.wall_velocity = 1;
        fr.vx.assign(nvert, 0.0f); fr.vy.assign(nvert, 0.0f); fr.vz.assign(nvert, 0.0f);
    }
    try { sh.BuildMesh(fr); }
    catch (const std::exception &e) { std::fprintf(stderr, "refused: %s\n", e.what()); return 3; }
    f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    std::fwrite(sh.type.data(), 1, sh.type.size(), f);
    static_assert(sizeof(int) == 4, "the owners are written as int32");
    std::fwrite(sh.owner.data(), 4, sh.owner.size(), f);
    std::fclose(f);
    return 0;
}
