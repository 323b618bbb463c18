/* Moving Shape3D meshes on x-slabs: two entries beside fs3d_update_nodes_shape3d (fs3d.h) and fs3d_update_nodes_shape3d_vel
 * (fs3d_mesh_walls.h), and one test aid, in libfs3d_hip.so.  An extension header in the manner of fs3d_slab_geometry.h, which
 * includes it: the headers before it keep the sets of functions they declared, and the mesh entries of fs3d.h and
 * fs3d_mesh_walls.h keep refusing an x-slab (FS3D_ERR_UNSUPPORTED, "single context only"). */
#ifndef FS3D_SLAB_MESH_H
#define FS3D_SLAB_MESH_H

#include "fs3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tables of a mesh's geometry for the planes [x_offset, x_offset + dimx) of the global grid, with the voxelisation and the
 * flood fill on the device.  The fill is global -- NODE_OUT spreads from cell (0,0,0) of the GLOBAL grid -- and the staging buffer
 * of a slab update already holds the byte arrays of the global grid (the X lines need them): every rank voxelises and fills the
 * global grid on its own device and asks nothing of a neighbour.  No communication, as for the entries of fs3d_slab_geometry.h:
 * the call waits for no peer, so it is the same for a lone slab context, a member of an in-process group and an RCCL rank; the
 * caller makes it on every rank between the same two time steps.  A whole-grid context (x_offset 0, dimx == dimx_global, no group)
 * is accepted too and ends with what fs3d_update_nodes_shape3d[_vel] builds.
 *
 * Arguments and checks are those of fs3d_update_nodes_shape3d and fs3d_update_nodes_shape3d_vel; the vertices are in GLOBAL grid
 * coordinates.  FS3D_OPT_MESH_VOXELS selects the reference's rasteriser or the conservative overlap test; the _vel entry needs the
 * conservative one.  Every refusal of the mesh itself (NULL array, no upload yet, an index outside the vertex list, a vertex that
 * is not finite or lies past the coordinate bound, _vel without the conservative option, a velocity or wallT that is not finite)
 * comes before the geometry is given up: the context is unchanged and nothing is counted.
 *
 * Result: after FS3D_OK the context holds exactly what a fresh context of the same (x_offset, dimx, dimx_global) holds after
 * fs3d_upload_nodes of the global nodes of the twin (shape3d.nodes_of / FillShape3DNodes of host/Shape3D.h; the _vel entry: with
 * its wall velocities and wallT) -- tables, node values and n_seg_out, byte for byte: the result clause of fs3d_update_nodes_slab.
 *
 * The rest of the contract is that of fs3d_update_nodes_slab, line for line: only after a first fs3d_upload_nodes; a geometry
 * refused after the kernels ran -- a scan line of the reference rasteriser past its bound; a shared FREE cell cannot occur, the
 * walls are NOSLIP -- leaves no geometry until an update or upload succeeds; layers, options and params are untouched; the call is
 * counted in CreateSegments and its device time is in fs3d_last_update_device_ms; nothing is allocated or freed after a
 * context's second call (the first brings the mesh buffers and, for _vel, the owner array -- 4 bytes per cell of the SLAB; a later
 * call with a larger mesh grows the mesh buffers).  A refusal's message starts with the entry's own name.
 *
 * Cost: rasterisation and flood fill run over the GLOBAL grid and are repeated on every rank, so that part of the device time does
 * not shrink with the number of ranks -- the price of asking nothing of a neighbour.  The node kernel and the tables work on
 * the slab's planes.  What travels is the mesh, 12 bytes per vertex (24 with velocities) and the index list when it changes,
 * against 3 bytes per global cell and the value planes for a host voxelisation followed by fs3d_update_nodes_slab.
 *
 * Not provided: a _dev form; a fill shared between the ranks of a group; shipping less than the global byte arrays. */
fs3d_status fs3d_update_nodes_shape3d_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, int nvert, const int *tri, int ntri,
                                           double baseT, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape3d_vel_slab(fs3d_ctx *ctx, const float *x, const float *y, const float *z, const float *wx, const float *wy,
                                               const float *wz, int nvert, const int *tri, int ntri, double baseT, double wallT,
                                               int n_seg_out[3]);

/* Test aid: fs3d_flood_fill_dev of fs3d.h for the GLOBAL grid, from any context -- the fill the two entries above run.
 * type_inout: dimx_global * dimy * dimz node types on the context's device, filled in place from global cell (0,0,0). */
fs3d_status fs3d_flood_fill_global_dev(fs3d_ctx *ctx, uint8_t *type_inout);

#ifdef __cplusplus
}
#endif
#endif /* FS3D_SLAB_MESH_H */
