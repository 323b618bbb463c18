"""Time statistics of the fields: what FS3D_OPT_TIME_STATS accumulates and what fs3d_get_layer, fs3d_get_layer_rows and
fs3d_get_layer_dev sample while FS3D_OPT_OUTPUT_SOURCE is 1, 2 or 3.

TimeStats is the definition of the rule; the kernels of csrc/kernels_stats.hip equal it bit for bit (every operation below is one
IEEE double operation, none is fused, and a cell asks nothing of a neighbour, so no order is left free).  The reference has no
counterpart: every record it writes is one instant.

Accumulation, once per time step, with x each of U, V, W, T of FS3D_LAYER_CUR after the step and `types` the node types of that
moment -- on the NODE_IN cells only:
    n += 1          (uint32)
    S1 += double(x)
    S2 += double(x) * double(x)          (mode 2)
and the window's step count N += 1.  Cells are counted by the type they have at each step: a geometry may move inside a window.

Read-out, per cell, all in double, each operation rounded once; R is the fields' type:
    n >= 1:  m = S1 / double(n)
        source 1, mean            Q = R(m)
        source 2, variance        v = S2 / double(n) - m * m, 0 where v < 0, Q = R(v)      (population variance over the n steps)
        source 3, fluid fraction  Q_T = R(double(n) / double(N)), Q_U = Q_V = Q_W = 0
    n == 0:  source 1: the value the cell holds in FS3D_LAYER_CUR now (walls show their node values as in every record);
             sources 2 and 3: 0.
The record rule of the three entries then runs on Q in place of `next`: the 99999 stamp on the cells that are NODE_OUT now, the
gather, and layer_output.py's filter and vector where those options are set.

Rounding of the mean: S1 is a recursive double sum of n terms, so |S1 - sum x| <= (n - 1) u sum |x| / (1 - (n - 1) u) with
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4), the division adds one relative u, and the rounding to
R one relative half-ulp of R.  mean_bound returns that bound.  The variance is the textbook one-pass formula: it cancels where
the mean is large against the spread (relative error about 2 u (m^2 / v)), is clamped at 0, and is exactly 0 for a constant field whose
square is exact in double (every fp32 value; S2 / n = x^2 and m * m = x^2 as long as n * x and n * x^2 are exact).

Not provided: covariances (Reynolds stresses), a stride (every k-th step), a history of cells that are NODE_OUT now, the 2D solver.
"""
import numpy as np

from .grids import NODE_IN

MEAN, VARIANCE, FRACTION = 1, 2, 3
SOURCES = {"next": 0, "mean": MEAN, "variance": VARIANCE, "fraction": FRACTION}


class TimeStats:
    """One window.  mode 1: first moments; mode 2: first and second moments."""

    def __init__(self, shape, mode=2):
        if mode not in (1, 2):
            raise ValueError("mode is 1 (first moments) or 2 (first and second moments)")
        self.shape, self.mode = tuple(shape), mode
        self.reset()

    def reset(self):
        """A new window: N = 0, every sum zero (what every fs3d_set_option(FS3D_OPT_TIME_STATS, ..) does)"""
        self.N = 0
        self.n = np.zeros(self.shape, np.uint32)
        self.S1 = [np.zeros(self.shape, np.float64) for _ in range(4)]
        self.S2 = [np.zeros(self.shape, np.float64) for _ in range(4)] if self.mode == 2 else None

    def add(self, fields, types):
        """One accumulated step: fields = U, V, W, T of `cur` after the step, types = the node types of that moment"""
        fluid = np.asarray(types) == NODE_IN
        assert fluid.shape == self.shape
        self.n[fluid] += np.uint32(1)
        with np.errstate(all="ignore"):
            for v in range(4):
                x = np.asarray(fields[v])[fluid].astype(np.float64)
                self.S1[v][fluid] = self.S1[v][fluid] + x
                if self.mode == 2:
                    self.S2[v][fluid] = self.S2[v][fluid] + x * x
        self.N += 1

    def layer(self, source, cur_fields):
        """Q of `source` (1 mean, 2 variance, 3 fluid fraction): four arrays of cur_fields' dtype, before the 99999 stamp"""
        if source not in (MEAN, VARIANCE, FRACTION):
            raise ValueError("source is 1 (mean), 2 (variance) or 3 (fluid fraction)")
        if source == VARIANCE and self.mode < 2:
            raise ValueError("the variance needs mode 2")
        if self.N == 0:
            raise ValueError("the window holds no step")
        R = np.asarray(cur_fields[0]).dtype
        seen = self.n >= 1
        dn = self.n[seen].astype(np.float64)
        out = []
        with np.errstate(all="ignore"):
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
