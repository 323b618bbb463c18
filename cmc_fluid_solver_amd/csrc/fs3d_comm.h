// Multi-GPU plumbing (RCCL, or the in-process transport) behind fs3d_comm_init / fs3d_comm_init_local: halo planes of the x-slab
// decomposition and the two-scalar all-reduce of EvalDivError.
#pragma once
#include "fs3d_common.h"

void fs3d_comm_destroy(fs3d_ctx *c);
// exchange the boundary x-planes of the first nfields fields of layer buffer `buf`
// with the slab neighbours (ScalarField3D::syncHalos, TimeLayer3D.h:272-335). No-op for one rank.
fs3d_status fs3d_comm_halo_exchange(fs3d_ctx *c, int buf, int nfields);
// The whole halo of one round of the fresh-cell fill (kernels_geom.hip) in ONE grouped exchange: per neighbour the boundary plane of
// the four fields of layer buffer `buf`, as fs3d_comm_halo_exchange moves them, and one plane of round tags (bytes) each way.  `tag`
// addresses the first owned plane of a byte array laid out as a field: a ghost plane in front of it and one behind the last.
// No-op for one rank.
fs3d_status fs3d_comm_fill_exchange(fs3d_ctx *c, int buf, uint8_t *tag);
// The same grouped exchange for any four fields laid out as a layer buffer's (`base`: the ghost plane below field 0, `fstride`
// elements from field to field) and any four planes of bytes: the own first and last plane go out, the neighbours' come in.  The
// collective result records (FS3D_OPT_OUTPUT_SLABS) move the sampled layer -- `next` or the statistic layer -- and the node types
// of the planes at the cuts with it.  No-op for one rank.
struct fs3d_byte_planes { uint8_t *send_lo, *send_hi, *recv_lo, *recv_hi; };
fs3d_status fs3d_comm_layer_exchange(fs3d_ctx *c, void *base, long long fstride, const fs3d_byte_planes &b);
// in-place sum of two doubles on the device over all ranks (TimeLayer3D.h:630-637). No-op for one rank.
fs3d_status fs3d_comm_allreduce_sum2(fs3d_ctx *c, double *dev2);
// the same for n doubles.  EvalDivError of a group: every rank holds zeros but for its own planes' partial sums, so each sum has one
// non-zero term and is exact -- the result is the array a single context of the global grid computes
fs3d_status fs3d_comm_allreduce_sum(fs3d_ctx *c, double *dev, size_t n);
// one grouped transfer of elements [l0,l1) of each of `nrows` rows (row pitch `pitch` elements) to/from `peer`
fs3d_status fs3d_comm_xfer_rows(fs3d_ctx *c, void *dev, int nrows, size_t pitch, long long l0, long long l1, int peer, bool send);
// all-gather of `count` elements per rank: recv = [rank][count] (send may not alias recv); one grouped exchange
fs3d_status fs3d_comm_allgather(fs3d_ctx *c, const void *send, void *recv, size_t count);
// all-to-all of `count` elements per pair of ranks: block r of `send` goes to rank r, block r of `recv` comes from rank r (the own block is a
// device copy); one grouped exchange of point-to-point transfers -- one send and one receive per peer
fs3d_status fs3d_comm_alltoall(fs3d_ctx *c, const void *send, void *recv, size_t count);
extern "C" fs3d_status fs3d_comm_abort(fs3d_ctx *c);
