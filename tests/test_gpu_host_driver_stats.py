"""fs3d_run --time-stats: <prefix>_stats.nc holds the records the Python path takes from the same library (mean, variance, fluid
fraction through FS3D_OPT_OUTPUT_SOURCE), _res.nc is the file of the run without the word, and `GPU 2` writes the same statistics."""
import os
import re
import subprocess

import numpy as np
import pytest

from cmc_fluid_solver_amd import build as B
from cmc_fluid_solver_amd import capi, shape2d

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")
NSTEPS = 6
OD = (7, 6, 5)


def driver_case(tmp_path):
    """box_pipe (a 64^3 grid), the shipped config with a 7 x 6 x 5 output grid"""
    data, cfgf = (os.path.join(INPUTS, f) for f in ("box_pipe_2D_data.txt", "box_pipe_2D_config.txt"))
    text = open(cfgf).read()
    for name, v in zip(("out_gridx", "out_gridy", "out_gridz"), OD):
        line = [l for l in text.splitlines() if l.split() and l.split()[0] == name]
        assert len(line) == 1
        text = text.replace(line[0], "%s\t%d" % (name, v))
    cfgf = str(tmp_path / "config.txt")
    open(cfgf, "w").write(text)
    return data, cfgf


def run(driver, data, prefix, cfgf, words):
    return subprocess.run([driver, data, prefix, cfgf, "align"] + words + ["--steps", str(NSTEPS)], check=True, capture_output=True, text=True,
                          timeout=300).stdout


def without_times(out):
    """The driver's prints less the numbers a clock gave: the progress line's time left, the profiler table, the closing rate"""
    out = out.split("\nProfiling data")[0] + out[out.index("Sweep kernels:"):]
    out = re.sub(r"\([^()]* left\)", "", out)
    return re.sub(r"steps in [0-9.]+ s: [0-9.]+ Mcells/s", "steps", out)


def test_stats_file_holds_the_python_paths_records(built, tmp_path, monkeypatch):
    from scipy.io import netcdf_file
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    plain = run(driver, data, str(tmp_path / "plain"), cfgf, ["GPU"])
    out = run(driver, data, str(tmp_path / "var"), cfgf, ["GPU", "--time-stats", "variance"])
    lines = out.rstrip().splitlines()
    assert lines[-1] == "Time statistics: %d steps, mean, variance in %s_stats.nc" % (NSTEPS, tmp_path / "var")
    assert not os.path.exists(str(tmp_path / "plain_stats.nc"))
    # _res.nc and every print are those of the run without the word
    assert open(str(tmp_path / "var_res.nc"), "rb").read() == open(str(tmp_path / "plain_res.nc"), "rb").read()
    assert without_times("\n".join(lines[:-1])).replace("var_res.nc", "plain_res.nc") == without_times(plain.rstrip())
    # the Python path: the driver's loop, then the three sources
    nodes, cfg, dt = shape2d.load_case(data, cfgf, align=True)
    assert (cfg.outdimx, cfg.outdimy, cfg.outdimz) == OD
    s = capi.Solver(nodes, capi.fluid_params(np.float32, cfg.Re, cfg.Pr, cfg.lam), np.float32)
    s.set_option(capi.OPT_TIME_STATS, 2)
    for i in range(NSTEPS):
        s.UpdateBoundaries()
        s.TimeStep(np.float32(dt), cfg.num_global, cfg.num_local, i % 10 == 0)
        if i % cfg.out_time_steps == 0:
            s.GetLayer(OD)                                     # the driver's call: the stamp on `next`
    records = []
    for source in (1, 2, 3):
        s.set_option(capi.OPT_OUTPUT_SOURCE, source)
        records.append(s.GetLayer(OD))
    s.close()
    f = netcdf_file(str(tmp_path / "var_stats.nc"), "r", mmap=False)
    assert f.variables["u"].shape == (3,) + OD
    for r, (V, T) in enumerate(records):
        fV = np.stack([np.asarray(f.variables[nm][r], np.float64) for nm in "uvw"], axis=-1)
        fT = np.ascontiguousarray(f.variables["T"][r], np.float64)
        assert np.array_equal(fV, V.astype(np.float64)) and np.array_equal(fT, T), r
    f.close()
    V, T = records[2]
    fluid = T != 99999.0
    assert fluid.any() and (V[fluid] == 0).all() and ((T[fluid] == 0) | (T[fluid] == 1)).all() and (T[fluid] == 1).any()
    assert not np.array_equal(records[0][1], records[2][1]) and (records[1][0][fluid] >= 0).all()
    # `mean`: two records, the same mean and fraction
    out = run(driver, data, str(tmp_path / "mean"), cfgf, ["GPU", "--time-stats", "mean"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: %d steps, mean in %s_stats.nc" % (NSTEPS, tmp_path / "mean")
    g = netcdf_file(str(tmp_path / "mean_stats.nc"), "r", mmap=False)
    f = netcdf_file(str(tmp_path / "var_stats.nc"), "r", mmap=False)
    assert g.variables["u"].shape == (2,) + OD
    for nm in "uvwT":
        assert np.array_equal(g.variables[nm][0], f.variables[nm][0]) and np.array_equal(g.variables[nm][1], f.variables[nm][2]), nm
    f.close()
    g.close()


def test_two_slabs_write_the_same_statistics(built, tmp_path, monkeypatch):
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")                 # the bit-exact kernels: slabs equal the single context bit for bit
    driver = B.build_driver()
    data, cfgf = driver_case(tmp_path)
    run(driver, data, str(tmp_path / "one"), cfgf, ["GPU", "--time-stats", "variance"])
    out = run(driver, data, str(tmp_path / "two"), cfgf, ["GPU", "2", "--same-device", "--time-stats", "variance"])
    assert out.rstrip().splitlines()[-1] == "Time statistics: %d steps, mean, variance in %s_stats.nc" % (NSTEPS, tmp_path / "two")
    assert open(str(tmp_path / "two_res.nc"), "rb").read() == open(str(tmp_path / "one_res.nc"), "rb").read()
    stats = open(str(tmp_path / "two_stats.nc"), "rb").read()
    assert len(stats) > 1000 and stats == open(str(tmp_path / "one_stats.nc"), "rb").read()
