/* Moving geometry on x-slabs: two entries beside fs3d_update_nodes and fs3d_update_nodes_shape2d of fs3d.h (and one test aid), in libfs3d_hip.so.
 * The entries for a Shape3D mesh, beside fs3d_update_nodes_shape3d[_vel], are declared in fs3d_slab_mesh.h, which this header
 * includes: whoever includes this one has every slab entry.
 * An extension header: fs3d.h keeps the set of functions it declared before these existed, and its update entries keep refusing
 * an x-slab (FS3D_ERR_UNSUPPORTED, "single context only"). */
#ifndef FS3D_SLAB_GEOMETRY_H
#define FS3D_SLAB_GEOMETRY_H

#include "fs3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The tables of a new geometry for the planes [x_offset, x_offset + dimx) of the global grid, rebuilt on the device between two
 * time steps.  No communication: as fs3d_upload_nodes does, every rank takes the GLOBAL input and builds the tables of its own
 * planes from it, with kernels on its own stream.  The call waits for no peer, so it is the same for a lone slab context, a member
 * of an in-process group and an RCCL rank; the caller makes it on every rank between the same two time steps (and treats any
 * rank's failure as fatal for the group, as for every other call).  A whole-grid context (x_offset 0, dimx == dimx_global, no
 * group) is accepted too and ends with the tables fs3d_update_nodes builds.
 *
 *   fs3d_update_nodes_slab          host arrays over the global grid, exactly as fs3d_upload_nodes takes them.  The three byte
 *                                   arrays travel whole; of the four value arrays only the slab's planes are read.
 *   fs3d_update_nodes_shape2d_slab  the arguments and checks of fs3d_update_nodes_shape2d; the 2D arrays cover dimx_global x dimy
 *                                   columns.  The extrusion runs on the device: the byte arrays are written for all global columns,
 *                                   the value fields for the slab's planes.
 *
 * Result: after FS3D_OK the context holds exactly what a fresh context of the same (x_offset, dimx, dimx_global) holds after
 * fs3d_upload_nodes of the same arrays -- cell codes, dead lines (local: a slab whose piece of an X line holds only the line's END
 * cell is live), shared columns, the BOUND / VALVE list, the node values, stale_in_cells; n_seg_out[0] counts the segments of
 * the global X lines, [1] and [2] those of the slab's planes.  FS3D_ERR_UNSUPPORTED (a FREE cell that closes one segment and opens
 * the next) exactly when that upload would return it: such a cell on ANY global X line, or on a Y / Z line of the slab's planes.
 *
 * In every line the contract is that of fs3d_update_nodes*: only after a first fs3d_upload_nodes; a refusal that comes before the
 * geometry is given up (NULL array, no upload yet, a bad Shape2D source) leaves the context unchanged and counts nothing; a geometry
 * refused by the tables leaves no geometry until an update or upload succeeds; layers, options and params are untouched; the call
 * is counted in CreateSegments and its device time is in fs3d_last_update_device_ms.  Nothing is allocated or freed after a
 * context's first slab update (the BOUND / VALVE list is grow-only).
 *
 * Cost: the staging buffer of a slab context holds the three byte arrays of the GLOBAL grid -- 3 bytes per global cell,
 * allocated by the first slab update, never shrunk -- and every rank reads them for the X lines, so that pass does not shrink
 * with the number of ranks; everything else works on the slab's planes.
 *
 * Not provided: a _dev form of these entries; shipping less than the global byte arrays.  (A mesh on a slab is voxelised on the
 * device by the entries of fs3d_slab_mesh.h: the flood fill is global, so every rank runs it over the global grid in the staging
 * buffer described above.  fs3d_update_nodes_shape3d[_vel] themselves keep refusing a slab.) */
fs3d_status fs3d_update_nodes_slab(fs3d_ctx *ctx, const uint8_t *type, const uint8_t *bc_vel, const uint8_t *bc_temp,
                                   const void *vx, const void *vy, const void *vz, const void *T, int n_seg_out[3]);
fs3d_status fs3d_update_nodes_shape2d_slab(fs3d_ctx *ctx, const uint8_t *cell2d, const float *velx2d, const float *vely2d,
                                           const float *T2d, double dz, double depth, double depth_var, double baseT,
                                           int n_seg_out[3]);

/* Test and measurement aid, for any context with a geometry: the dead-line bytes of direction dir (0 X: [j][k], 1 Y: [i][k],
 * 2 Z: [i][j], i over the context's own planes) -- 1 where no cell of the context's piece of the line is NODE_IN or on a segment.
 * fs3d_geometry_info counts them; which lines they are is what a slab update has to get right for X, where the piece is not the
 * line.  n_lines_out (may be NULL) receives the number of lines; dead_out (may be NULL: the count alone) that many bytes. */
fs3d_status fs3d_geometry_dead_lines(fs3d_ctx *ctx, int dir, uint8_t *dead_out, long long *n_lines_out);

#ifdef __cplusplus
}
#endif

#include "fs3d_slab_mesh.h"

#endif /* FS3D_SLAB_GEOMETRY_H */
