"""Filtered and derived result records: what fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev return while
FS3D_OPT_OUTPUT_FILTER, FS3D_OPT_OUTPUT_VECTOR, FS3D_OPT_OUTPUT_GRADIENT or FS3D_OPT_OUTPUT_WALL is set.

layer_output is the definition of the rule; k_get_layer_box (csrc/kernels_output.hip) is held to it -- bit for bit wherever the double
sums are exact, to the rounding of one sum elsewhere.  The reference has no counterpart: its FilterToArrays (TimeLayer3D.h:819-924)
is the point sample, which is filter 0 with vector 0 here.

The source is `next` after the 99999 stamp on the NODE_OUT cells (Solver3D.cpp:21-25); the types are the context's current ones.

Box of output index i on an axis of g source cells and o samples (o = 0: o = g): lo = i*g // o, hi = max(lo + 1, (i+1)*g // o).
For o <= g the boxes partition the axis and each starts at the reference's sample cell; for o >= g every box is that one cell.

Per cell q = (a, b, c, T).  vector 0: (a, b, c) = (U, V, W).  vector 1: the vorticity in the fields' type R, central differences,
every operation rounded in R, two_dx = R(2) * R(dx):
  wx = (W[j+1] - W[j-1]) / two_dy - (V[k+1] - V[k-1]) / two_dz
  wy = (U[k+1] - U[k-1]) / two_dz - (W[i+1] - W[i-1]) / two_dx
  wz = (V[i+1] - V[i-1]) / two_dx - (U[j+1] - U[j-1]) / two_dy
on a NODE_IN cell whose six neighbours are inside the grid and not NODE_OUT (an OUT neighbour holds the stamp, not a velocity);
(99999, 99999, 99999) on a NODE_OUT cell, so the missing-value marker survives; (0, 0, 0) on every other cell.

vector INVARIANTS (FS3D_OPT_OUTPUT_GRADIENT 1; the constant is that option's id, 20: `vector` 2 stays refused here as
FS3D_OPT_OUTPUT_VECTOR 2 is by the library): the invariants of the velocity gradient, (a, b, c) = (div, Q, S:S), on the cells that carry a
vorticity (curl_defined, unchanged); 99999 and 0 elsewhere as above.  With a over the fields U, V, W (indices x, y, z), b over the
axes and h = R(0.5), every operation rounded once in R, in this order, nothing fused:
  g_ab = (u_a[b+1] - u_a[b-1]) / two_db                                  nine quotients
  div  = (g_xx + g_yy) + g_zz
  s_xy = h*(g_xy + g_yx)   s_xz = h*(g_xz + g_zx)   s_yz = h*(g_yz + g_zy)
  o_xy = h*(g_xy - g_yx)   o_xz = h*(g_xz - g_zx)   o_yz = h*(g_yz - g_zy)
  SS   = ((g_xx*g_xx + g_yy*g_yy) + g_zz*g_zz) + R(2)*((s_xy*s_xy + s_xz*s_xz) + s_yz*s_yz)       S:S, the strain rate (2 nu S:S is the dissipation)
  OO   = R(2)*((o_xy*o_xy + o_xz*o_xz) + o_yz*o_yz)                                                the rotation rate
  Q    = h*(OO - SS)                                                                               positive inside a vortex
A rigid rotation of rate w gives (0, w^2, 0), a plane shear of rate w (0, 0, w^2 / 2), a plane stretch (0, -w^2, 2 w^2), a uniform
dilatation of rate w (3 w, -3 w^2 / 2, 3 w^2).  On integer fields of magnitude up to 63 with power-of-two spacings every operation
is exact in fp32, so fp32 and fp64 agree value for value.

vector WALL_VECTOR / WALL_SCALARS (FS3D_OPT_OUTPUT_WALL 1 / 2; wall_loads is the rule): what the flow does to the wall, on the wall
cells.  A wall cell B (NODE_BOUND or NODE_VALVE) has the exposed face (d, s), axis d and s = -1 or +1, iff P = B + s*e_d is inside the
grid, NODE_IN and an INTERIOR row of direction d of the geometry tables (fs3d_tables.h line_kinds: its index along the line is >= 1
and a cell that is not NODE_IN lies beyond it) -- the faces where the solver imposes B's node value on the line through P.  A
carrier is a wall cell with at least one exposed face.  With A_x = R(dy)*R(dz), A_y = R(dx)*R(dz), A_z = R(dx)*R(dy), h_d = R(d_d),
nu = R(v_vis), kappa = R(t_vis), all sums from R(0), the exposed faces in the order x-, x+, y-, y+, z-, z+, every operation
rounded once in R, nothing fused:
  area = area + A_d
  velocity BC of B NOSLIP, each component c != d:   g = (F_c[P] - F_c[B]) / h_d ;  t = nu * g ;     sum_c = sum_c + A_d * t
  temperature BC of B NOSLIP:                       g = (T[P] - T[B]) / h_d ;      t = kappa * g ;  sum_q = sum_q + A_d * t
  tau_c = sum_c / area     q = sum_q / area     mag = sqrt((tau_x*tau_x + tau_y*tau_y) + tau_z*tau_z)
tau is the shear traction the fluid exerts on the wall (fluid moving +x over a wall at rest: tau_x > 0 on either side of the wall),
q > 0 is heat flowing into the wall; a FREE face adds its area and nothing else (an outflow face is a carrier with zero loads); the
wall's own value F[B] is read from the sampled layer, so a wall that carries a velocity gives the relative shear.  (a, b, c) is
tau (WALL_VECTOR) or (mag, q, area) (WALL_SCALARS) on the carriers, 99999 on NODE_OUT cells and 0 on every other cell.  For these
two modes the C of filter 1 below is the carriers of the box, not its NODE_IN cells: a coarse record shows the mean load of the
wall cells under each sample.  Not provided: second-order one-sided differences, the wall-normal viscous stress, a pressure-like
force, x-slabs.

filter 0: the sample is q of the cell (lo_x, lo_y, lo_z).
filter 1: with C the NODE_IN cells of the sample's box -- C empty: filter 0's sample (a wall value or 99999); else per quantity
m = (sum over C of (double)q) / (double)|C|, the sum in double in any order, one double division; outT = m and each outV component
is m rounded once to R.  With every o >= g filter 1 equals filter 0 bit for bit.  A field that is constant on NODE_IN comes out as
that constant wherever |C| times the constant is exact in double: in fp32 for every box of up to 2^29 cells (24 + 29 bits), in fp64 for constants of few
significant bits (else to the rounding of the sum).
"""
import math

import numpy as np

from .grids import BC_FREE, NODE_BOUND, NODE_IN, NODE_OUT, NODE_VALVE

MISSING_VALUE = 99999.0
POINT, BOX = 0, 1
VELOCITY, VORTICITY = 0, 1                                # the values of FS3D_OPT_OUTPUT_VECTOR
INVARIANTS = 20                                           # FS3D_OPT_OUTPUT_GRADIENT 1, which claims outV in the vector option's place
WALL_VECTOR, WALL_SCALARS = 221, 222                      # FS3D_OPT_OUTPUT_WALL (id 22) 1 and 2, which claim outV too


def boxes(g, o):
    """(lo, hi) of every output index of one axis: int64 arrays of o (or g, for o = 0) entries"""
    o = o or g
    i = np.arange(o, dtype=np.int64)
    lo = i * g // o
    return lo, np.maximum(lo + 1, (i + 1) * g // o)


def stamp(type, fields):
    """Copies of the four fields with 99999 on the NODE_OUT cells: what the entries leave in `next`"""
    out_cells = np.asarray(type) == NODE_OUT
    out = [np.array(f, copy=True) for f in fields]
    for f in out:
        f[out_cells] = MISSING_VALUE
    return out


def curl_defined(type):
    """The cells that carry a vorticity: NODE_IN, the six neighbours inside the grid and not NODE_OUT"""
    t = np.asarray(type)
    ok = np.zeros(t.shape, bool)
    not_out = t != NODE_OUT
    ok[1:-1, 1:-1, 1:-1] = (t[1:-1, 1:-1, 1:-1] == NODE_IN) & \
        not_out[:-2, 1:-1, 1:-1] & not_out[2:, 1:-1, 1:-1] & not_out[1:-1, :-2, 1:-1] & not_out[1:-1, 2:, 1:-1] & \
        not_out[1:-1, 1:-1, :-2] & not_out[1:-1, 1:-1, 2:]
    return ok


def vorticity(type, fields, spacing):
    """(wx, wy, wz) per cell as the rule gives them, in the fields' dtype; fields are the stamped U, V, W(, T)."""
    U, V, W = fields[:3]
    R = U.dtype.type
    two = [R(2) * R(d) for d in spacing]
    c = (slice(1, -1),) * 3

    def d(f, axis):                                       # f[+1] - f[-1] along axis, on the interior
        hi = [slice(1, -1)] * 3
        lo = [slice(1, -1)] * 3
        hi[axis], lo[axis] = slice(2, None), slice(None, -2)
        return f[tuple(hi)] - f[tuple(lo)]
    with np.errstate(all="ignore"):                       # differences against the stamp are computed and thrown away
        w = [d(W, 1) / two[1] - d(V, 2) / two[2], d(U, 2) / two[2] - d(W, 0) / two[0], d(V, 0) / two[0] - d(U, 1) / two[1]]
    ok = curl_defined(type)
    out_cells = np.asarray(type) == NODE_OUT
    res = []
    for comp in w:
        assert comp.dtype == U.dtype
        full = np.zeros(U.shape, U.dtype)
        full[c] = np.where(ok[c], comp, R(0))
        full[out_cells] = R(MISSING_VALUE)
        res.append(full)
    return res


def invariants(type, fields, spacing):
    """(div, Q, S:S) per cell as the rule gives them, in the fields' dtype; fields are the stamped U, V, W(, T)."""
    F = fields[:3]
    R = F[0].dtype.type
    two = [R(2) * R(d) for d in spacing]
    c = (slice(1, -1),) * 3
    h = R(0.5)

    def g(a, b):                                          # (u_a[b+1] - u_a[b-1]) / two_db, on the interior
        hi = [slice(1, -1)] * 3
        lo = [slice(1, -1)] * 3
        hi[b], lo[b] = slice(2, None), slice(None, -2)
        return (F[a][tuple(hi)] - F[a][tuple(lo)]) / two[b]
    with np.errstate(all="ignore"):                       # differences against the stamp are computed and thrown away
        gxx, gxy, gxz, gyx, gyy, gyz, gzx, gzy, gzz = [g(a, b) for a in range(3) for b in range(3)]
        div = (gxx + gyy) + gzz
        sxy, sxz, syz = h * (gxy + gyx), h * (gxz + gzx), h * (gyz + gzy)
        oxy, oxz, oyz = h * (gxy - gyx), h * (gxz - gzx), h * (gyz - gzy)
        SS = ((gxx * gxx + gyy * gyy) + gzz * gzz) + R(2) * ((sxy * sxy + sxz * sxz) + syz * syz)
        OO = R(2) * ((oxy * oxy + oxz * oxz) + oyz * oyz)
        Q = h * (OO - SS)
    ok = curl_defined(type)
    out_cells = np.asarray(type) == NODE_OUT
    res = []
    for comp in (div, Q, SS):
        assert comp.dtype == F[0].dtype
        full = np.zeros(F[0].shape, F[0].dtype)
        full[c] = np.where(ok[c], comp, R(0))
        full[out_cells] = R(MISSING_VALUE)
        res.append(full)
    return res


def node_arrays(nodes_or_arrays):
    """(type, bc_vel, bc_temp) of a grids.Nodes object or of a triple of arrays"""
    n = nodes_or_arrays
    if hasattr(n, "bc_vel"):
        return np.asarray(n.type), np.asarray(n.bc_vel), np.asarray(n.bc_temp)
    if isinstance(n, (tuple, list)) and len(n) == 3:
        return tuple(np.asarray(a) for a in n)
    raise ValueError("the wall loads need the node types and both boundary-condition arrays: a Nodes object or (type, bc_vel, bc_temp)")


def interior_rows(type, d):
    """The INTERIOR rows of direction d, indexed (i, j, k): NODE_IN, index along the line >= 1, a cell that is not NODE_IN beyond it"""
    ty = np.moveaxis(np.asarray(type), d, 2)
    s = np.arange(ty.shape[2])
    notin = ty != NODE_IN
    lst = np.where(notin, s, -1).max(axis=2)
    return np.moveaxis(~notin & (s >= 1) & (s < lst[..., None]), 2, d)


def exposed_faces(type):
    """Six bool arrays, in the order x-, x+, y-, y+, z-, z+: the wall cells B whose face towards B + s*e_d is exposed"""
    t = np.asarray(type)
    wall = (t == NODE_BOUND) | (t == NODE_VALVE)
    faces = []
    for d in range(3):
        inter = np.moveaxis(interior_rows(t, d), d, 0)
        for s in (-1, 1):
            f = np.zeros_like(inter)
            if s < 0:
                f[1:] = inter[:-1]
            else:
                f[:-1] = inter[1:]
            faces.append(np.moveaxis(f, 0, d) & wall)
    return faces


class WallLoads:
    """What wall_loads returns: carrier (bool) and tau (three arrays), mag, q, area in the fields' dtype, 0 off the carriers"""

    def __init__(self, carrier, tau, mag, q, area):
        self.carrier, self.tau, self.mag, self.q, self.area = carrier, tau, mag, q, area


def wall_loads(nodes_or_arrays, fields, spacing, nu, kappa):
    """The wall shear stress and the wall heat flux per wall cell as the rule gives them (module docstring), from the fields U, V, W, T
    of the sampled layer."""
    type, bc_vel, bc_temp = node_arrays(nodes_or_arrays)
    F = [np.asarray(f) for f in fields[:4]]
    R = F[0].dtype.type
    h = [R(d) for d in spacing]
    A = [h[1] * h[2], h[0] * h[2], h[0] * h[1]]
    nu, kappa = R(nu), R(kappa)
    vel_ns, temp_ns = bc_vel != BC_FREE, bc_temp != BC_FREE
    area = np.zeros(type.shape, F[0].dtype)
    sums = [np.zeros(type.shape, F[0].dtype) for _ in range(4)]
    faces = exposed_faces(type)
    with np.errstate(all="ignore"):
        for n, face in enumerate(faces):
            d, s = n // 2, (-1, 1)[n % 2]
            area = np.where(face, area + A[d], area)
            for c in range(4):
                if c == d:
                    continue
                fp = np.roll(F[c], -s, axis=d)             # F_c[P] at B (the wrapped entries are never on a face)
                g = (fp - F[c]) / h[d]
                t = (kappa if c == 3 else nu) * g
                on = face & (temp_ns if c == 3 else vel_ns)
                sums[c] = np.where(on, sums[c] + A[d] * t, sums[c])
        carrier = faces[0] | faces[1] | faces[2] | faces[3] | faces[4] | faces[5]
        one = np.where(carrier, area, R(1))
        tau = [np.where(carrier, sums[c] / one, R(0)) for c in range(3)]
        q = np.where(carrier, sums[3] / one, R(0))
        mag = np.sqrt((tau[0] * tau[0] + tau[1] * tau[1]) + tau[2] * tau[2])
    for a in tau + [q, mag, area]:
        assert a.dtype == F[0].dtype
    return WallLoads(carrier, tau, mag, q, area)


def wall_quantities(nodes_or_arrays, fields, vector, spacing, nu, kappa):
    """(a, b, c) of the modes WALL_VECTOR and WALL_SCALARS per cell, and the carriers"""
    type = node_arrays(nodes_or_arrays)[0]
    w = wall_loads(nodes_or_arrays, fields, spacing, nu, kappa)
    R = w.mag.dtype.type
    res = []
    for comp in (w.tau if vector == WALL_VECTOR else [w.mag, w.q, w.area]):
        full = np.where(w.carrier, comp, R(0))
        full[type == NODE_OUT] = R(MISSING_VALUE)
        res.append(full)
    return res, w.carrier


def cell_quantities(type, fields, vector=VELOCITY, spacing=None, nu=None, kappa=None):
    """q = (a, b, c, T) per cell from the fields as they are before the call (the stamp is applied here).  The wall modes take a
    Nodes object or (type, bc_vel, bc_temp) as `type`, and nu and kappa."""
    if vector in (WALL_VECTOR, WALL_SCALARS):
        if spacing is None or nu is None or kappa is None:
            raise ValueError("the wall loads need the grid's spacing (dx, dy, dz), nu and kappa")
        st = stamp(node_arrays(type)[0], fields)
        return wall_quantities(type, st, vector, spacing, nu, kappa)[0] + [st[3]]
    st = stamp(type, fields)
    if vector == VELOCITY:
        return st
    if vector not in (VORTICITY, INVARIANTS):
        raise ValueError("vector is 0 (velocity), 1 (vorticity) or INVARIANTS (the velocity-gradient invariants)")
    if spacing is None:
        raise ValueError("the vorticity and the invariants need the grid's spacing (dx, dy, dz)")
    return (vorticity if vector == VORTICITY else invariants)(type, st, spacing) + [st[3]]


def layer_output(type, fields, outdims=(0, 0, 0), filter=POINT, vector=VELOCITY, spacing=None, exact_sum=False, nu=None, kappa=None,
                 members=None):
    """The record of one call: (outV [odx, ody, odz, 3] in the fields' dtype, outT [odx, ody, odz] float64).
    fields: U, V, W, T of `next` before the call, four arrays [dimx, dimy, dimz] of one float dtype (not modified).
    exact_sum: the box sums by math.fsum, so that a mean carries the rounding of its division alone (the yardstick of a bound);
    otherwise numpy's double sum.
    The wall modes take a Nodes object or (type, bc_vel, bc_temp) as `type`, and nu and kappa; the C of their filter 1 is the carriers.
    members: the C of filter 1 as a bool array, in place of the mode's own (the statistic layers of FS3D_OPT_OUTPUT_WALL 3 and 4)."""
    if filter not in (POINT, BOX):
        raise ValueError("filter is 0 (point) or 1 (box)")
    q = cell_quantities(type, fields, vector, spacing, nu, kappa)
    wall_mode = vector in (WALL_VECTOR, WALL_SCALARS)
    type = node_arrays(type)[0] if wall_mode else np.asarray(type)
    R = q[0].dtype
    dims = type.shape
    ax = [boxes(g, o) for g, o in zip(dims, outdims)]
    sel = np.ix_(*[lo for lo, _ in ax])
    outV = np.stack([f[sel] for f in q[:3]], axis=-1)
    outT = q[3][sel].astype(np.float64)
    if filter == POINT or all((hi - lo == 1).all() for lo, hi in ax):      # (the mean of one value: (R)((double)q / 1.0) = q)
        return outV, outT
    if members is not None:
        fluid = np.asarray(members, bool)
    elif wall_mode:
        t3 = type
        fluid = np.zeros(t3.shape, bool)
        for f in exposed_faces(t3):
            fluid |= f
    else:
        fluid = type == NODE_IN
    for i, (x0, x1) in enumerate(zip(*ax[0])):
        for j, (y0, y1) in enumerate(zip(*ax[1])):
            for k, (z0, z1) in enumerate(zip(*ax[2])):
                box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                m = fluid[box]
                n = int(m.sum())
                if n == 0:
                    continue
                mean = []
                for f in q:
                    vals = f[box][m].astype(np.float64)
                    mean.append((math.fsum(vals) if exact_sum else float(vals.sum())) / float(n))
                outV[i, j, k] = np.array(mean[:3], np.float64).astype(R)
                outT[i, j, k] = mean[3]
    return outV, outT


# ---- the record on x-slabs (FS3D_OPT_OUTPUT_SLABS): every slab reduces its own planes, the partial sums of the rows at the cuts travel ----
# `cuts`: the planes [x0, x1) of every rank, in rank order, a partition of [0, gx).  The statement works from the GLOBAL arrays: q of
# a cell is the global rule's (the library gets the same bits from its own planes, the neighbours' boundary planes and their types).

def owned_rows(cuts, rank, gx, odx):
    """Rows [i0, i1) of the record that rank writes: those whose box begins in its planes (slab.out_rows)"""
    odx = odx or gx
    x0, x1 = cuts[rank]
    return -(-x0 * odx // gx), -(-x1 * odx // gx)


def straddling_rows(cuts, gx, odx):
    """The rows whose box holds planes of more than one slab, ascending: at most len(cuts) - 1, whatever the width of a box"""
    lo, hi = boxes(gx, odx)
    rows = []
    for x0, _ in cuts[1:]:
        for i in np.nonzero((lo < x0) & (hi > x0))[0]:
            if int(i) not in rows:
                rows.append(int(i))
    return sorted(rows)


def slab_partials(type, fields, cuts, rank, outdims=(0, 0, 0), filter=POINT, vector=VELOCITY, spacing=None):
    """What one rank computes before anything travels: ((i0, i1), outV [i1 - i0, ody, odz, 3], outT [i1 - i0, ody, odz], partials).
    The owned rows that straddle no cut are finished (the others are NaN); partials: {straddling row: float64 [5, ody, odz]} for
    EVERY straddling row of the group -- the four double sums and the count over the NODE_IN cells of the box that lie in the rank's
    own planes, zeros where its planes miss the box.  filter 0 has no straddling row: a sample is one cell, and its owner holds it."""
    type = np.asarray(type)
    q = cell_quantities(type, fields, vector, spacing)
    R = q[0].dtype
    gx = type.shape[0]
    ax = [boxes(g, o) for g, o in zip(type.shape, outdims)]
    od = [len(lo) for lo, _ in ax]
    x0s, x1s = cuts[rank]
    i0, i1 = owned_rows(cuts, rank, gx, od[0])
    strad = straddling_rows(cuts, gx, od[0]) if filter == BOX else []
    outV = np.full((i1 - i0, od[1], od[2], 3), np.nan, R)
    outT = np.full((i1 - i0, od[1], od[2]), np.nan, np.float64)
    partials = {i: np.zeros((5, od[1], od[2]), np.float64) for i in strad}
    fluid = type == NODE_IN
    for i in sorted(set(range(i0, i1)) | set(strad)):
        x0, x1 = max(int(ax[0][0][i]), x0s), min(int(ax[0][1][i]), x1s)       # the box, clipped to the slab's planes
        if x0 >= x1:
            continue
        for j, (y0, y1) in enumerate(zip(*ax[1])):
            for k, (z0, z1) in enumerate(zip(*ax[2])):
                box = (slice(x0, x1), slice(y0, y1), slice(z0, z1))
                m = fluid[box] if filter == BOX else np.zeros((x1 - x0, y1 - y0, z1 - z0), bool)
                n = int(m.sum())
                sums = [float(f[box][m].astype(np.float64).sum()) for f in q]
                if i in partials:
                    partials[i][:, j, k] = sums + [float(n)]
                elif n:
                    outV[i - i0, j, k] = np.array([s / float(n) for s in sums[:3]], np.float64).astype(R)
                    outT[i - i0, j, k] = sums[3] / float(n)
                else:
                    outV[i - i0, j, k] = [f[x0, y0, z0] for f in q[:3]]
                    outT[i - i0, j, k] = np.float64(q[3][x0, y0, z0])
    return (i0, i1), outV, outT, partials


def finish_slabs(type, fields, cuts, per_rank, outdims=(0, 0, 0), vector=VELOCITY, spacing=None):
    """The global record from every rank's slab_partials: the partials of a straddling row are added in rank order, then one division
    and one rounding, or the point sample of the cell (lo_x, lo_y, lo_z) where no rank counted a NODE_IN cell -- written, as in the
    library, by the row's owner, whose planes hold that cell."""
    type = np.asarray(type)
    q = cell_quantities(type, fields, vector, spacing)
    R = q[0].dtype
    ax = [boxes(g, o) for g, o in zip(type.shape, outdims)]
    od = [len(lo) for lo, _ in ax]
    outV, outT = np.full(od + [3], np.nan, R), np.full(od, np.nan, np.float64)
    for (i0, i1), V, T, _ in per_rank:
        outV[i0:i1], outT[i0:i1] = V, T
    for i in per_rank[0][3]:
        owner = [r for r, ((i0, i1), _, _, _) in enumerate(per_rank) if i0 <= i < i1]
        x0 = int(ax[0][0][i])
        assert len(owner) == 1 and cuts[owner[0]][0] <= x0 < cuts[owner[0]][1]
        total = np.zeros_like(per_rank[0][3][i])
        for p in per_rank:
            total = total + p[3][i]
        for j, y0 in enumerate(ax[1][0]):
            for k, z0 in enumerate(ax[2][0]):
                n = total[4, j, k]
                if n:
                    outV[i, j, k] = (total[:3, j, k] / n).astype(R)
                    outT[i, j, k] = total[3, j, k] / n
                else:
                    outV[i, j, k] = [f[x0, y0, z0] for f in q[:3]]
                    outT[i, j, k] = np.float64(q[3][x0, y0, z0])
    return outV, outT


def box_kinds(type, outdims):
    """Per sample: 0 every cell of the box NODE_IN, 1 mixed, 2 no NODE_IN and the sample cell a wall (NODE_BOUND / NODE_VALVE),
    3 no NODE_IN and the sample cell NODE_OUT.  int8 [odx, ody, odz]; test aid."""
    type = np.asarray(type)
    ax = [boxes(g, o) for g, o in zip(type.shape, outdims)]
    kinds = np.empty([len(lo) for lo, _ in ax], np.int8)
    for i, (x0, x1) in enumerate(zip(*ax[0])):
        for j, (y0, y1) in enumerate(zip(*ax[1])):
            for k, (z0, z1) in enumerate(zip(*ax[2])):
                t = type[x0:x1, y0:y1, z0:z1]
                n = int((t == NODE_IN).sum())
                kinds[i, j, k] = 0 if n == t.size else 1 if n else 3 if type[x0, y0, z0] == NODE_OUT else 2
    return kinds
