"""No GPU: the driver word --slab-output-filter (host/fs3d_run.cpp) against the recording stand-in of the library
(tests/driver_calls.py, tests/fs3d_stub.cpp).  With GPU n, `box` sets FS3D_OPT_OUTPUT_SLABS (19) and FS3D_OPT_OUTPUT_FILTER (12) on
every slab before the first step; with one GPU it is --output-filter; a run without the word makes no new call."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import driver_calls as D  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build(str(tmp_path_factory.mktemp("driver_output_slabs")))


def run(exe, tmp_path, tag, words):
    return D.run_case(exe, D._case(D.B, words), str(tmp_path / tag))


def test_the_word_sets_both_options_on_every_slab_before_the_first_step(exe, tmp_path):
    r = run(exe, tmp_path, "slabs", "GPU 2 --same-device --slab-output-filter box --steps 3")
    assert r["returncode"] == 0, r["stderr"]
    assert len(r["logs"]) == 2, "one call log per context"
    for name, log in r["logs"].items():
        lines = log.splitlines()
        first_step = min(k for k, l in enumerate(lines) if l.startswith("fs3d_time_step"))
        slabs, box = lines.index("fs3d_set_option 19 1"), lines.index("fs3d_set_option 12 1")
        assert slabs < box < first_step, name
        assert sum(l.startswith("fs3d_set_option 19") for l in lines) == 1 and sum(l.startswith("fs3d_get_layer_rows") for l in lines) >= 1
    assert r["files"]["out_res.nc"]
    plain = run(exe, tmp_path, "plain", "GPU 2 --same-device --steps 3")
    for log in plain["logs"].values():
        assert "fs3d_set_option 19" not in log and "fs3d_set_option 12" not in log
    # `point` is the default sample: no call either
    point = run(exe, tmp_path, "point", "GPU 2 --same-device --slab-output-filter point --steps 3")
    assert point["returncode"] == 0 and point["logs"] == plain["logs"] and point["files"] == plain["files"]


def test_with_one_gpu_the_word_is_output_filter_box(exe, tmp_path):
    a = run(exe, tmp_path, "slab_word", "GPU --slab-output-filter box --steps 3")
    b = run(exe, tmp_path, "plain_word", "GPU --output-filter box --steps 3")
    assert a["returncode"] == b["returncode"] == 0, a["stderr"] + b["stderr"]
    assert a["logs"] == b["logs"] and a["files"] == b["files"] and a["stdout"] == b["stdout"]
    assert all("fs3d_set_option 19" not in log and "fs3d_set_option 12 1" in log for log in a["logs"].values())


def test_the_statistics_records_take_the_word_too(exe, tmp_path):
    r = run(exe, tmp_path, "stats", "GPU 2 --same-device --slab-output-filter box --time-stats mean --steps 3")
    assert r["returncode"] == 0, r["stderr"]
    assert r["files"]["out_stats.nc"]
    for log in r["logs"].values():
        lines = log.splitlines()
        source = lines.index("fs3d_set_option 15 1")
        assert lines.index("fs3d_set_option 19 1") < source and any(l.startswith("fs3d_get_layer_rows") for l in lines[source:])
        assert "fs3d_set_option 19 0" not in log and "fs3d_set_option 12 0" not in log, "the filter stays on for the statistics records"


def test_the_words_argument_is_checked_and_the_plain_word_is_still_refused_on_slabs(exe, tmp_path):
    r = run(exe, tmp_path, "gauss", "GPU 2 --same-device --slab-output-filter gauss")
    assert r["returncode"] != 0 and "--output-filter: point or box" in r["stderr"] and not r["logs"]
    r = run(exe, tmp_path, "plain_box", "GPU 2 --same-device --output-filter box")
    assert r["returncode"] != 0 and "--output-filter box: single GPU only" in r["stderr"] and not r["logs"]
