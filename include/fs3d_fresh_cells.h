/* Fresh cells of a moving geometry: the entries that fill the cells an update turned NODE_IN from their fluid neighbours, beside
 * the moving-geometry entries of fs3d.h (which declares the option, FS3D_OPT_FRESH_CELLS), in libfs3d_hip.so.
 * An extension header: fs3d.h keeps the set of functions it declared before these existed. */
#ifndef FS3D_FRESH_CELLS_H
#define FS3D_FRESH_CELLS_H

#include "fs3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What a cell holds when a wall moves off it and it becomes NODE_IN.
 * No reference counterpart (its per-step grid->Prepare(t) is commented out, FluidSolver3D.cpp:237).  Without these entries a cell
 * that turns NODE_IN starts from what its layer holds: (0, 0, 0, baseT) where it was NODE_OUT, the wall's node values where it was
 * NODE_BOUND / NODE_VALVE -- for a Shape3D mesh T = 0 against baseT in the fluid, in a shell of cells, every step.
 * The rule (cmc_fluid_solver_amd/fresh_cells.py fill_fresh_cells is its numpy twin, and the kernels equal it bit for bit): with
 * prev_type the node types before the update and the context's code table giving them now, a cell is a DONOR if it is NODE_IN in
 * both, FRESH if it is NODE_IN now and was not, and otherwise neither read nor written.  The fill runs in rounds r = 1, 2, ..: every
 * fresh cell still unfilled looks at its six neighbours in the order i-1, i+1, j-1, j+1, k-1, k+1 (outside the grid: skipped); a
 * neighbour counts if it is a donor or was filled in a round BEFORE r; with n >= 1 of them each of the four fields of `layer` becomes
 * (x1 + .. + xn) / (real)n -- summed in that order, every addition and the one division rounded in the context's precision, no fused
 * multiply-add, no reciprocal -- and the cell counts as filled in round r.  A round reads only the state before it, so nothing
 * depends on the order of the cells.  The fill ends after the first round that fills nothing or after max_rounds rounds
 * (0 = 250, the largest value; outside 0 .. 250: FS3D_ERR_INVALID).  Fresh cells that no chain of fresh cells joins to a donor keep
 * what they hold.  Every filled value lies between the smallest and the largest donor value of its field.
 * info[0] fresh cells, [1] filled, [2] rounds that filled at least one cell, [3] fresh cells left unfilled.
 *
 * fs3d_fill_fresh_cells_dev, the stateless form: prev_type_dev holds dimx*dimy*dimz node types on the context's device (aligned
 * to 8 bytes: 8 cells per thread in the classifying pass; else cell by cell, same results).
 * fs3d_fill_fresh_cells reads the snapshot of FS3D_OPT_FRESH_CELLS and returns FS3D_ERR_INVALID without a valid one: the option is
 * off (or was when the last update ran), no update has succeeded since the last fs3d_upload_nodes, or the update before the last
 * one failed and left no geometry to take the types from.
 * Both refuse before any launch, the context unchanged: a NULL argument, a bad layer, a bad max_rounds, no nodes yet --
 * FS3D_ERR_INVALID; an x-slab or group member -- FS3D_ERR_UNSUPPORTED (single context only: a slab would need its neighbour's
 * plane).  Both work on the context's stream and return synchronised.  The round tag of every cell (one byte), the compact list
 * of the fresh cells and the counter words are allocated by the first fill, kept, and only the list grows: counted in
 * fs3d_geometry_info entry 13.  In a time loop the fill of FS3D_LAYER_CUR goes between the update and fs3d_update_boundaries.
 * fs3d_last_fill_device_ms: device time of the last fill (as fs3d_last_update_device_ms: while fs3d_enable_timing is on, else 0);
 * for fs3d_fill_fresh_cells it includes the snapshot's copy kernel, which runs inside the update call but is not part of the
 * update's device time. */
fs3d_status fs3d_fill_fresh_cells_dev(fs3d_ctx *ctx, const uint8_t *prev_type_dev, int layer, int max_rounds, long long info[4]);
fs3d_status fs3d_fill_fresh_cells(fs3d_ctx *ctx, int layer, int max_rounds, long long info[4]);
fs3d_status fs3d_last_fill_device_ms(fs3d_ctx *ctx, float *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* FS3D_FRESH_CELLS_H */
