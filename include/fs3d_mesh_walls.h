/* Walls of a Shape3D mesh that carry the mesh's velocity: two entries beside the mesh entries of fs3d.h, in libfs3d_hip.so.
 * An extension header: fs3d.h keeps the set of functions it declared before these existed. */
#ifndef FS3D_MESH_WALLS_H
#define FS3D_MESH_WALLS_H

#include "fs3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Walls that carry the mesh's velocity and a temperature: fs3d_update_nodes_shape3d / fs3d_voxelize_shape3d_dev with a velocity per
 * vertex, wx, wy, wz (float, nvert each, in the solver's velocity units: what host/Shape3D.h SubFrameVelocity(t) and
 * shape3d.Shape3D.subframe_velocity(t) return), and wallT.  The reference reads a velocity per vertex and interpolates it
 * (Grid3D.cpp:915), then drops it in RasterPolygon / RasterLine: its walls are at rest whatever the mesh does, and a wall that moves
 * never pushes the fluid.  Here, with the conservative voxelisation only (FS3D_OPT_MESH_VOXELS set to 1), whose overlap test defines it:
 *   owner     of a NODE_BOUND cell: the triangle of smallest index whose overlap test sets the cell (order-free: an integer
 *             minimum).  Where several triangles overlap a cell the choice is arbitrary; the velocity field of a mesh is continuous
 *             across shared vertices, so another choice moves the value by the velocity gradient times a cell.
 *   weights   float64 from the fp32 vertices, local to the cell's corner: the barycentric coordinates of the orthogonal projection
 *             of the cell's centre onto the owner's plane, clamped at 0 and normalised; a degenerate owner gives the clamped
 *             parameter of the projection onto its longest edge (cmc_fluid_solver_amd/shape3d.py states every operation).
 *   nodes     NODE_BOUND: bc_vel = bc_temp = NOSLIP, v = (w0 W0 + w1 W1) + w2 W2 per component rounded once to real,
 *             T = (real)(float)wallT; every other cell as in the entries above (v = 0, T = (real)(float)baseT).
 * The nodes equal those of shape3d.nodes_of(.., wall_v, wall_T) and of host/Shape3D.h FillShape3DNodes byte for byte.  With all
 * velocities zero and wallT = 0 the seven arrays equal those of fs3d_update_nodes_shape3d / fs3d_voxelize_shape3d_dev byte for byte.
 * In every line the contract is that of those two entries (only after a first upload, single context only -- FS3D_ERR_UNSUPPORTED
 * for an x-slab --, a refused geometry leaves no geometry, the update is counted in CreateSegments and its device time is in
 * fs3d_last_update_device_ms).  More refusals, FS3D_ERR_INVALID before anything is launched, the context unchanged:
 * FS3D_OPT_MESH_VOXELS other than 1, a NULL velocity array, a velocity or wallT that is not finite.
 * The owner array (4 bytes per cell) is allocated by the first call of one of these two entries, never in steady state. */
fs3d_status fs3d_update_nodes_shape3d_vel(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                          const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                          double wallT, int n_seg_out[3]);
fs3d_status fs3d_voxelize_shape3d_vel_dev(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx,
                                          const float *wy, const float *wz, int nvert, const int *tri, int ntri, double baseT,
                                          double wallT, uint8_t *type_out, uint8_t *bc_vel_out, uint8_t *bc_temp_out,
                                          void *vx_out, void *vy_out, void *vz_out, void *T_out);

#ifdef __cplusplus
}
#endif
#endif /* FS3D_MESH_WALLS_H */
