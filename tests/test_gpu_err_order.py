"""FS3D_OPT_ERR_ORDER = 1: EvalDivError sums its per-cell terms in cell order, as the CPU path's loop does (TimeLayer3D.h:604-628), so
that on the bit-exact kernels the reported error equals the oracle's bit for bit -- not only to the 1e-12 of the parallel summation."""
import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids

pytestmark = pytest.mark.gpu
PARAMS = (200.0, 0.72, 1.4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_serial_order_error_equals_the_oracle_bit_for_bit(built, dtype):
    from oracle import oracle as O
    g = grids.box_with_obstacle(24, 20, 28, h=0.04)
    params = capi.fluid_params(dtype, *PARAMS)
    s = capi.Solver(g, params, dtype)
    s.set_option(capi.OPT_SWEEP_KERNEL, capi.SWEEP_EXACT)
    o = O.Oracle(g, params, dtype)
    base = [np.ascontiguousarray(a, dtype) for a in (g.vx, g.vy, g.vz, g.T)]
    cur = grids.perturb(base, seed=7)
    s.upload_layer(capi.LAYER_CUR, cur)
    for v in range(4):
        o.set_field(O.L_CUR, v, cur[v])
    par, ser = [], []
    for step in range(3):
        s.UpdateBoundaries(); o.update_boundaries()
        rc, eo = o.time_step(0.1, 2, 2, True)
        s.set_option(capi.OPT_ERR_ORDER, 1)
        es = s.TimeStep(0.1, 2, 2, True)
        assert rc == 0 and es == eo, (step, es, eo)
        e1, n1 = s.eval_div_error(capi.LAYER_CUR)
        s.set_option(capi.OPT_ERR_ORDER, 0)
        e0, n0 = s.eval_div_error(capi.LAYER_CUR)
        eo2, no = o.eval_div_error(O.L_CUR)
        print(step, es, eo, e0, e1)
        assert e1 == eo2 and n1 == n0 == no
        assert abs(e0 - eo2) <= 1e-12 * abs(eo2)          # the default order: close, not necessarily equal
        par.append(e0); ser.append(e1)
    s.close(); o.close()


def test_serial_order_is_refused_on_a_slab(built):
    g = grids.box(16, 12, 12)
    s = capi.Solver(g, capi.fluid_params(np.float32, *PARAMS), np.float32, x_range=(0, 8))
    s.set_option(capi.OPT_ERR_ORDER, 1)
    with pytest.raises(capi.Fs3dError) as ei:
        s.eval_div_error(capi.LAYER_CUR)
    assert ei.value.status == capi.ERR_UNSUPPORTED
    s.set_option(capi.OPT_ERR_ORDER, 0)
    s.eval_div_error(capi.LAYER_CUR)
    s.close()
