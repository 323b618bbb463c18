"""The event pairs of a time step (fs3d_enable_timing / fs3d_profiler_events): every launch group of time_step_enqueue opens one pair and
closes it, so the counts per event of the reference's Profiler vocabulary are fixed by (G, L) and the merge form, and every pair has a
recorded end event -- its time is a finite number >= 0.  Counts read off time_step_enqueue (single context: no syncHalos):
  fused merge (default)   SolveSegments_{Z,Y,X} = G*L each; CopyLayer = 1 (cur -> next on the boundary list); MergeLayer = 0 (in the sweeps)
  FS3D_OPT_FUSE_MERGE 0   SolveSegments_{Z,Y,X} = G*L each; CopyLayer = 2 (+ cur -> temp); MergeLayer = G*(3L + 1)
  both                    EvalDivError = 1, UpdateBoundaries = 1 (the call before the step; collected with the step's events)"""
import math

import numpy as np
import pytest

from cmc_fluid_solver_amd import capi, grids

pytestmark = pytest.mark.gpu
PARAMS = (200.0, 0.72, 1.4)
G, L = 2, 2
SWEEPS = {"SolveSegments_Z": G * L, "SolveSegments_Y": G * L, "SolveSegments_X": G * L}
EXPECTED = {
    1: dict(SWEEPS, CopyLayer=1, MergeLayer=0, EvalDivError=1, UpdateBoundaries=1, syncHalos=0),
    0: dict(SWEEPS, CopyLayer=2, MergeLayer=G * (3 * L + 1), EvalDivError=1, UpdateBoundaries=1, syncHalos=0),
}


@pytest.mark.parametrize("fuse", [1, 0])
def test_event_counts_of_a_time_step(built, fuse):
    g = grids.box_with_obstacle(20, 16, 18)
    s = capi.Solver(g, capi.fluid_params(np.float32, *PARAMS), np.float32)
    s.set_option(capi.OPT_FUSE_MERGE, fuse)
    s.enable_timing(True)
    for step in (1, 2):                                    # the second step adds the same counts again
        s.UpdateBoundaries()
        s.TimeStep(0.1, G, L, True)
        ev = s.profiler_events()
        print(fuse, step, ev)
        for name, n in EXPECTED[fuse].items():
            assert ev[name][1] == step * n, (name, ev[name], step * n)
        for name, (ms, n) in ev.items():
            assert math.isfinite(ms) and ms >= 0.0, (name, ms)
    s.close()
