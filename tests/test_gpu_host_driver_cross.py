"""fs3d_run --time-stats variance --time-covariances [--time-stats-every K]: <prefix>_stats.nc holds five records -- mean, variance,
Reynolds stresses, turbulent heat flux, fluid fraction -- equal to those the Python path takes from the same library
(FS3D_OPT_TIME_STATS_CROSS, FS3D_OPT_OUTPUT_MOMENT, FS3D_OPT_TIME_STATS_EVERY), _res.nc and every other print are those of the run
without the words, and `GPU 2` writes the same bytes.  The case and its helpers: test_gpu_host_driver_stats.py."""
import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, shape2d
from cmc_fluid_solver_amd import time_stats as TS

from test_gpu_host_driver_stats import NSTEPS, OD, driver_case, run, without_times  # noqa: E402

pytestmark = pytest.mark.gpu

LAYERS = ((1, 0), (2, 0), (2, 1), (2, 2), (3, 0))              # (source, moment) of the five records, in the file's order


def python_records(data, cfgf, every):
    """The driver's loop on the Python path, then the five layers; and the twin's layers, fed the `cur` of every step"""
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    assert (cfg.outdimx, cfg.outdimy, cfg.outdimz) == OD
    s = capi.Solver(nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    s.set_option(capi.OPT_TIME_STATS, 2)
    s.set_option(capi.OPT_TIME_STATS_CROSS, 1)
    if every > 1:
        s.set_option(capi.OPT_TIME_STATS_EVERY, every)
    twin = TS.TimeStats(s.dims, 2, cross=True, every=every)
    types = np.asarray(nodes.type)
    for i in range(NSTEPS):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        twin.add(s.download_layer(capi.LAYER_CUR), types)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(OD)                                     # the driver's call: the stamp on `next`
    records, twins = [], []
    cur = s.download_layer(capi.LAYER_CUR)
    for source, moment in LAYERS:
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        s.set_option(capi.OPT_OUTPUT_MOMENT, moment)
        records.append(s.GetLayer(OD))
        twins.append(twin.layer(source, cur, moment))
    s.close()
    return records, twins, types, twin.N


def file_records(path):
    from scipy.io import netcdf_file
    f = netcdf_file(path, "r", mmap=False)
    n = f.variables["u"].shape[0]
    assert f.variables["u"].shape == (n,) + OD
    out = [(np.stack([np.asarray(f.variables[nm][r], np.float64) for nm in "uvw"], axis=-1), np.ascontiguousarray(f.variables["T"][r], np.float64))
           for r in range(n)]
    f.close()
    return out


def test_covariance_records_equal_the_python_paths(built, tmp_path, monkeypatch):
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    plain = run(driver, data, str(tmp_path / "plain"), cfgf, ["GPU"])
    out = run(driver, data, str(tmp_path / "cov"), cfgf, ["GPU", "--time-stats", "variance", "--time-covariances"])
    lines = out.rstrip().splitlines()
    assert lines[-1] == "Time statistics: %d steps, mean, variance, covariances in %s_stats.nc" % (NSTEPS, tmp_path / "cov")
    # _res.nc and every other print are those of the run without the words
    assert open(str(tmp_path / "cov_res.nc"), "rb").read() == open(str(tmp_path / "plain_res.nc"), "rb").read()
    assert without_times("\n".join(lines[:-1])).replace("cov_res.nc", "plain_res.nc") == without_times(plain.rstrip())
    records, twins, types, N = python_records(data, cfgf, 1)
    assert N == NSTEPS
    got = file_records(str(tmp_path / "cov_stats.nc"))
    assert len(got) == 5
    for r, ((fV, fT), (V, T)) in enumerate(zip(got, records)):
        assert np.array_equal(fV, V.astype(np.float64)) and np.array_equal(fT, T), r
    # the records are what they are called: stresses of both signs beside a non-negative k, and the variance of T beside the fluxes
    fluid = records[4][1] != 99999.0
    assert fluid.any() and (records[2][1][fluid] >= 0).all() and (records[2][1][fluid] > 0).any()
    assert (records[2][0][fluid] != 0).any()
    assert np.array_equal(records[3][1], records[1][1]), "var_T is the T of the variance record"
    # the variance file of the run without --time-covariances: records 0, 1 and 4 of this one
    run(driver, data, str(tmp_path / "var"), cfgf, ["GPU", "--time-stats", "variance"])
    old = file_records(str(tmp_path / "var_stats.nc"))
    assert len(old) == 3
    for a, b in zip(old, (got[0], got[1], got[4])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # GPU 2 --same-device: the same bytes
    out2 = run(driver, data, str(tmp_path / "two"), cfgf, ["GPU", "2", "--same-device", "--time-stats", "variance", "--time-covariances"])
    assert out2.rstrip().splitlines()[-1] == "Time statistics: %d steps, mean, variance, covariances in %s_stats.nc" % (NSTEPS, tmp_path / "two")
    assert open(str(tmp_path / "two_res.nc"), "rb").read() == open(str(tmp_path / "cov_res.nc"), "rb").read()
    stats = open(str(tmp_path / "two_stats.nc"), "rb").read()
    assert len(stats) > 1000 and stats == open(str(tmp_path / "cov_stats.nc"), "rb").read()


def test_every_second_step_gives_three_steps_and_the_twins_records(built, tmp_path, monkeypatch):
    from test_gpu_time_stats import gather
    from cmc_fluid_solver_amd import layer_output as LO
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    out = run(driver, data, str(tmp_path / "e2"), cfgf, ["GPU", "--time-stats", "variance", "--time-covariances", "--time-stats-every", "2"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: 3 steps, mean, variance, covariances in %s_stats.nc" % (tmp_path / "e2")
    records, twins, types, N = python_records(data, cfgf, 2)
    assert N == 3
    got = file_records(str(tmp_path / "e2_stats.nc"))
    assert len(got) == 5
    for r, ((fV, fT), (V, T), Q) in enumerate(zip(got, records, twins)):
        assert np.array_equal(fV, V.astype(np.float64)) and np.array_equal(fT, T), r
        eV, eT = gather(LO.stamp(types, Q), OD)
        assert np.array_equal(V, eV, equal_nan=True) and np.array_equal(T, eT, equal_nan=True), r
    # a stride without covariances: the three records, the same mean, variance and fraction
    out = run(driver, data, str(tmp_path / "v2"), cfgf, ["GPU", "--time-stats", "variance", "--time-stats-every", "2"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: 3 steps, mean, variance in %s_stats.nc" % (tmp_path / "v2")
    old = file_records(str(tmp_path / "v2_stats.nc"))
    assert len(old) == 3
    for a, b in zip(old, (got[0], got[1], got[4])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
