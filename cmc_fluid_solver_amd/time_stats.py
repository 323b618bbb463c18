"""Time statistics of the fields: what FS3D_OPT_TIME_STATS (with FS3D_OPT_TIME_STATS_CROSS and FS3D_OPT_TIME_STATS_EVERY)
accumulates and what fs3d_get_layer, fs3d_get_layer_rows and fs3d_get_layer_dev sample while FS3D_OPT_OUTPUT_SOURCE is 1, 2 or 3
(source 2: the second-moment layer FS3D_OPT_OUTPUT_MOMENT chooses).

TimeStats is the definition of the rule; the kernels of csrc/kernels_stats.hip equal it bit for bit (every operation below is one
IEEE double operation, none is fused, and a cell asks nothing of a neighbour, so no order is left free).  The reference has no
counterpart: every record it writes is one instant.

The stride.  A window counts its candidate steps s = 1, 2, ..: every time step that succeeds (a diverged one is no candidate).
Candidate s is accumulated if and only if (s - 1) % every == 0, so the first step of a window always counts; on the other steps
nothing happens.  N and the per-cell n count accumulated steps only.

Accumulation, once per accumulated step, with x each of U, V, W, T of FS3D_LAYER_CUR after the step and `types` the node types of that
moment -- on the NODE_IN cells only:
    n += 1          (uint32)
    S1 += double(x)
    S2 += double(x) * double(x)          (mode 2)
    S_ab += double(x_a) * double(x_b)    (mode 2 with cross; the pairs 0..5: uv, uw, vw, uT, vT, wT)
and the window's step count N += 1.  The product is rounded once, the addition once.  Cells are counted by the type they have at
each step: a geometry may move inside a window.

Gradient sums (FS3D_OPT_TIME_STATS_GRAD 1; TimeStats(gradients=True, spacing=...)): every accumulated step also evaluates the
invariants of the velocity gradient, layer_output.invariants, on FS3D_LAYER_CUR -- (div, Q, S:S) in R, from a cell's six neighbours
-- and on the cells that carry them in the geometry of that moment (layer_output.curl_defined):
    ng += 1         (uint32)
    G_div += double(div),  G_Q += double(Q),  G_SS += double(SS)      each addition rounded once
They are quadratic in the gradient, so the time mean of S:S is not S:S of the mean field: it has to be summed step by step.
Whole-grid contexts only.  Every set of the option opens a new window.
Read-out (FS3D_OPT_OUTPUT_GRADIENT 2 with source 1; gradient_layer): Q_U, Q_V, Q_W = R(G_div / double(ng)), R(G_Q / double(ng)),
R(G_SS / double(ng)) where ng >= 1 and R(0) where ng = 0; Q_T is source 1's.  The record rule then runs on Q as a velocity layer.

Wall sums (FS3D_OPT_TIME_STATS_WALL 1; TimeStats(wall=True, spacing=..., nu=..., kappa=...)): every accumulated step also evaluates
the wall loads, layer_output.wall_loads, on FS3D_LAYER_CUR in the geometry of that moment, and on each carrier:
    nw += 1         (uint32)
    W_x += double(tau_x),  W_y += double(tau_y),  W_z += double(tau_z),  W_mag += double(mag),  W_q += double(q)      each addition rounded once
The traction is linear in the fields, its magnitude is not: the time-averaged wall shear stress (TAWSS, the mean of |tau|) and the
oscillatory shear index (OSI) have to be summed step by step.  Whole-grid contexts only.  Every set of the option opens a new window.
Read-out (FS3D_OPT_OUTPUT_WALL 3 and 4 with source 1; wall_layer), in double with dn = double(nw), nw >= 1:
    3:  Q_U, Q_V, Q_W = R(W_x / dn), R(W_y / dn), R(W_z / dn)
    4:  m_c = W_c / dn ;  mm = sqrt((m_x*m_x + m_y*m_y) + m_z*m_z) ;  tawss = W_mag / dn
        osi = 0.5 * (1 - mm / tawss) where tawss > 0, else 0; 0 where that is negative
        Q_U, Q_V, Q_W = R(tawss), R(W_q / dn), R(osi)
and R(0) where nw = 0; Q_T is source 1's.  The record rule then runs on Q as a velocity layer; the C of its filter 1 is the cells with
nw >= 1 that are not NODE_OUT now.

Read-out, per cell, all in double, each operation rounded once; R is the fields' type:
    n >= 1:  dn = double(n), m_a = S1_a / dn
        source 1, mean            Q = R(m)
        source 2, moment 0, variance   var_a = S2_a / dn - m_a * m_a, 0 where that is negative, Q = R(var)   (population variance
                                       over the n steps)
        source 2, moment 1, Reynolds stresses   cov(a, b) = S_ab / dn - m_a * m_b, NOT clamped (a covariance may be negative):
                                       Q_U = R(cov(u, v)), Q_V = R(cov(u, w)), Q_W = R(cov(v, w)),
                                       Q_T = R(0.5 * ((var_u + var_v) + var_w)), the turbulent kinetic energy
        source 2, moment 2, turbulent heat flux   Q_U = R(cov(u, T)), Q_V = R(cov(v, T)), Q_W = R(cov(w, T)), Q_T = R(var_T)
        source 3, fluid fraction  Q_T = R(double(n) / double(N)), Q_U = Q_V = Q_W = 0
    n == 0:  source 1: the value the cell holds in FS3D_LAYER_CUR now (walls show their node values as in every record);
             sources 2 (every moment) and 3: 0.
The record rule of the three entries then runs on Q in place of `next`: the 99999 stamp on the cells that are NODE_OUT now, the
gather, and layer_output.py's filter where that option is set (the vector option: moment 0 only, the curl of a stress layer means
nothing).

Rounding of the mean: S1 is a recursive double sum of n terms, so |S1 - sum x| <= (n - 1) u sum |x| / (1 - (n - 1) u) with
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), the division adds one relative u, and the rounding to
R one relative half-ulp of R.  mean_bound returns that bound.  The variance is the textbook one-pass formula: it cancels where
the mean is large against the spread (relative error about 2 u (m^2 / v)), is clamped at 0, and is exactly 0 for a constant field whose
square is exact in double (every fp32 value; S2 / n = x^2 and m * m = x^2 as long as n * x and n * x^2 are exact).  The one-pass
covariance carries the same caveat: S_ab / n and m_a * m_b cancel where the means are large against the co-fluctuation (absolute
error about 2 u |m_a m_b|), it is not clamped, and it is exactly 0 for two constant fields whose product is exact in double (every
pair of fp32 values) as long as n * x_a, n * x_b and n * x_a * x_b are exact.

Not provided: third moments, covariances with the vorticity, second moments of the invariants, gradient sums and wall sums on x-slabs, wall sums on a compact list of wall cells, a history of cells that are NODE_OUT now, the 2D solver.
"""
import numpy as np

from .grids import NODE_IN
from .layer_output import curl_defined, invariants, node_arrays, wall_loads

MEAN, VARIANCE, FRACTION = 1, 2, 3
SOURCES = {"next": 0, "mean": MEAN, "variance": VARIANCE, "fraction": FRACTION}
MOMENTS = {"variance": 0, "stress": 1, "heatflux": 2}
PAIRS = ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 3))       # uv, uw, vw, uT, vT, wT
MAX_EVERY = 2 ** 20


class TimeStats:
    """One window.  mode 1: first moments; mode 2: first and second moments; cross (mode 2 only, without effect in mode 1): the six
    cross sums as well; every: the stride of the accumulated steps."""

    def __init__(self, shape, mode=2, cross=False, every=1, gradients=False, spacing=None, wall=False, nu=None, kappa=None):
        if mode not in (1, 2):
            raise ValueError("mode is 1 (first moments) or 2 (first and second moments)")
        if int(every) != every or not 1 <= every <= MAX_EVERY:
            raise ValueError("every is an integer from 1 to 2^20")
        if gradients and spacing is None:
            raise ValueError("the gradient sums need the grid's spacing (dx, dy, dz)")
        self.shape, self.mode, self.cross, self.every = tuple(shape), mode, bool(cross) and mode == 2, int(every)
        if wall and (spacing is None or nu is None or kappa is None):
            raise ValueError("the wall sums need the grid's spacing (dx, dy, dz), nu and kappa")
        self.gradients, self.spacing = bool(gradients), None if spacing is None else tuple(spacing)
        self.wall, self.nu, self.kappa = bool(wall), nu, kappa
        self.reset()

    def reset(self):
        """A new window: N = 0, no candidate step yet, every sum zero (what every fs3d_set_option of FS3D_OPT_TIME_STATS,
        FS3D_OPT_TIME_STATS_CROSS and FS3D_OPT_TIME_STATS_EVERY does)"""
        self.N = 0
        self.candidates = 0
        self.n = np.zeros(self.shape, np.uint32)
        self.S1 = [np.zeros(self.shape, np.float64) for _ in range(4)]
        self.S2 = [np.zeros(self.shape, np.float64) for _ in range(4)] if self.mode == 2 else None
        self.SX = [np.zeros(self.shape, np.float64) for _ in PAIRS] if self.cross else None
        self.ng = np.zeros(self.shape, np.uint32) if self.gradients else None
        self.G = [np.zeros(self.shape, np.float64) for _ in range(3)] if self.gradients else None      # div, Q, S:S
        self.nw = np.zeros(self.shape, np.uint32) if self.wall else None
        self.W = [np.zeros(self.shape, np.float64) for _ in range(5)] if self.wall else None           # tau_x, tau_y, tau_z, mag, q

    def add(self, fields, types):
        """One candidate step: fields = U, V, W, T of `cur` after the step, types = the node types of that moment (with wall sums: a
        Nodes object or (type, bc_vel, bc_temp) of that moment).  Returns whether the stride let it be accumulated."""
        self.candidates += 1
        if (self.candidates - 1) % self.every:
            return False
        nodes = types
        if self.wall or hasattr(types, "bc_vel"):
            types = node_arrays(types)[0]
        fluid = np.asarray(types) == NODE_IN
        assert fluid.shape == self.shape
        self.n[fluid] += np.uint32(1)
        with np.errstate(all="ignore"):
            x = [np.asarray(fields[v])[fluid].astype(np.float64) for v in range(4)]
            for v in range(4):
                self.S1[v][fluid] = self.S1[v][fluid] + x[v]
                if self.mode == 2:
                    self.S2[v][fluid] = self.S2[v][fluid] + x[v] * x[v]
            if self.cross:
                for p, (a, b) in enumerate(PAIRS):
                    self.SX[p][fluid] = self.SX[p][fluid] + x[a] * x[b]
            if self.gradients:
                ok = curl_defined(types)
                inv = invariants(types, [np.asarray(f) for f in fields[:3]], self.spacing)
                self.ng[ok] += np.uint32(1)
                for v in range(3):
                    self.G[v][ok] = self.G[v][ok] + inv[v][ok].astype(np.float64)
            if self.wall:
                w = wall_loads(nodes, [np.asarray(f) for f in fields[:4]], self.spacing, self.nu, self.kappa)
                on = w.carrier
                self.nw[on] += np.uint32(1)
                for v, a in enumerate(w.tau + [w.mag, w.q]):
                    self.W[v][on] = self.W[v][on] + a[on].astype(np.float64)
        self.N += 1
        return True

    def wall_layer(self, cur_fields, which):
        """Q of FS3D_OPT_OUTPUT_WALL `which`: 3 the time mean of tau, 4 (tawss, mean q, osi), in place of U, V, W (0 where nw = 0)
        and source 1's T, four arrays of cur_fields' dtype, before the 99999 stamp"""
        if not self.wall:
            raise ValueError("the window holds no wall sums")
        if which not in (3, 4):
            raise ValueError("which is 3 (the mean traction) or 4 (tawss, the mean heat flux, osi)")
        if self.N == 0:
            raise ValueError("the window holds no step")
        R = np.asarray(cur_fields[0]).dtype
        seen = self.nw >= 1
        dn = self.nw[seen].astype(np.float64)
        with np.errstate(all="ignore"):
            m = [self.W[v][seen] / dn for v in range(5)]
            if which == 3:
                vals = m[:3]
            else:
                mm = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                tawss = m[3]
                osi = np.where(tawss > 0.0, 0.5 * (1.0 - mm / np.where(tawss > 0.0, tawss, 1.0)), 0.0)
                vals = [tawss, m[4], np.where(osi < 0.0, 0.0, osi)]
            out = []
            for v in range(3):
                q = np.zeros(self.shape, R)
                q[seen] = vals[v].astype(R)
                out.append(q)
        return out + [self.layer(MEAN, cur_fields)[3]]

    def gradient_layer(self, cur_fields):
        """Q of FS3D_OPT_OUTPUT_GRADIENT 2: the time means of div, Q and S:S in place of U, V, W (0 where ng = 0) and source 1's T,
        four arrays of cur_fields' dtype, before the 99999 stamp"""
        if not self.gradients:
            raise ValueError("the window holds no gradient sums")
        if self.N == 0:
            raise ValueError("the window holds no step")
        R = np.asarray(cur_fields[0]).dtype
        seen = self.ng >= 1
        dn = self.ng[seen].astype(np.float64)
        out = []
        with np.errstate(all="ignore"):
            for v in range(3):
                q = np.zeros(self.shape, R)
                q[seen] = (self.G[v][seen] / dn).astype(R)
                out.append(q)
        return out + [self.layer(MEAN, cur_fields)[3]]

    def layer(self, source, cur_fields, moment=0):
        """Q of `source` (1 mean, 2 second moments, 3 fluid fraction): four arrays of cur_fields' dtype, before the 99999 stamp.
        moment, read for source 2 only: 0 the variances, 1 the Reynolds stresses and k, 2 the heat fluxes and var_T"""
        if source not in (MEAN, VARIANCE, FRACTION):
            raise ValueError("source is 1 (mean), 2 (variance) or 3 (fluid fraction)")
        if source == VARIANCE and self.mode < 2:
            raise ValueError("the variance needs mode 2")
        if source == VARIANCE and moment not in (0, 1, 2):
            raise ValueError("moment is 0 (variance), 1 (stress) or 2 (heatflux)")
        if source == VARIANCE and moment and not self.cross:
            raise ValueError("the covariances need mode 2 with cross")
        if self.N == 0:
            raise ValueError("the window holds no step")
        R = np.asarray(cur_fields[0]).dtype
        seen = self.n >= 1
        dn = self.n[seen].astype(np.float64)
        out = []
        with np.errstate(all="ignore"):
            if source == VARIANCE and moment:
                m = [self.S1[v][seen] / dn for v in range(4)]

                def var(v):
                    mm = m[v] * m[v]
                    d = self.S2[v][seen] / dn - mm
                    return np.where(d < 0.0, 0.0, d)

                def cov(p):
                    a, b = PAIRS[p]
                    mab = m[a] * m[b]
                    return self.SX[p][seen] / dn - mab
                if moment == 1:
                    vals = [cov(0), cov(1), cov(2), 0.5 * ((var(0) + var(1)) + var(2))]
                else:
                    vals = [cov(3), cov(4), cov(5), var(3)]
                for v in range(4):
                    q = np.zeros(self.shape, R)
                    q[seen] = vals[v].astype(R)
                    out.append(q)
                return out
            for v in range(4):
                q = np.zeros(self.shape, R)
                if source == MEAN:
                    q[...] = cur_fields[v]
                    q[seen] = (self.S1[v][seen] / dn).astype(R)
                elif source == VARIANCE:
                    m = self.S1[v][seen] / dn
                    mm = m * m
                    var = self.S2[v][seen] / dn - mm
                    q[seen] = np.where(var < 0.0, 0.0, var).astype(R)
                elif v == 3:
                    q[seen] = (dn / np.float64(self.N)).astype(R)
                out.append(q)
        return out


def mean_bound(abs_sum, n, dtype):
    """Bound of |Q - exact mean| for the mean of n values whose absolute values sum to abs_sum (the derivation: module docstring)"""
    u = 2.0 ** -53
    g = (n - 1) * u / (1.0 - (n - 1) * u)
    exact_scale = abs_sum / n
    in_double = exact_scale * (g + u * (1.0 + g))
    return in_double + (exact_scale + in_double) * float(np.finfo(dtype).eps) / 2
