"""host/fs3d_run.cpp pinned call by call, without a GPU: the driver is compiled against a recording stand-in for libfs3d_hip.so
(tests/fs3d_stub.cpp) and, for every command line of the matrix in tests/driver_calls.py, held to tests/golden/driver_calls/<case>.json:
return code, stderr, stdout with the host-clock numbers masked, the call log of every context (order, arguments, a hash of every
array handed over) and the sha256 of _res.nc and _stats.nc.  The goldens were made by tests/golden/make_driver_calls.py from the
driver as it stood before its single-GPU loop and its x-slab loop became one; they are not made again when the driver changes."""
import json
import os
import re

import pytest

import driver_calls as D


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return D.build(str(tmp_path_factory.mktemp("driver_calls_bin")))


@pytest.fixture(scope="module")
def exe_tsan(tmp_path_factory):
    return D.build(str(tmp_path_factory.mktemp("driver_calls_tsan")), sanitize=True)


def _golden(name):
    with open(os.path.join(D.GOLDEN, name + ".json")) as f:
        return json.load(f)


def _assert_equals_golden(got, want):
    assert got["returncode"] == want["returncode"], got["stderr"]
    assert got["stderr"] == want["stderr"]
    assert got["stdout"] == want["stdout"]
    assert sorted(got["logs"]) == sorted(want["logs"])
    for ctx in want["logs"]:
        assert got["logs"][ctx].splitlines() == want["logs"][ctx].splitlines(), "context at x_offset " + ctx
    assert got["files"] == want["files"]


@pytest.mark.parametrize("name", list(D.CASES))
def test_driver_calls_equal_the_golden(exe, name, tmp_path):
    case = D.CASES[name]
    got = D.run_case(exe, case, str(tmp_path / "run"))
    _assert_equals_golden(got, _golden(name))
    if name in D.REFUSALS:
        assert got["returncode"] == 255 and D.REFUSALS[name][1] in got["stderr"] and not got["logs"]
    if case["fail"]:
        # the run ends by itself (run_case has a timeout) with the failing rank's own message
        entry, offset, nth = case["fail"].split(":")
        assert got["returncode"] == 255
        text = "stub: %s failed on the context at x_offset %s, call %s" % (entry, offset, nth)
        assert got["stderr"] == "\n\nCaught exception:\n%s%s\n\nTerminating...\n" % ("fs3d_create: " if entry == "fs3d_create" else "", text)
        assert "another slab thread failed" not in got["stderr"] + got["stdout"]


def test_goldens_are_those_of_the_matrix_and_small():
    files = sorted(os.listdir(D.GOLDEN))
    assert files == sorted(name + ".json" for name in D.CASES)
    assert sum(os.path.getsize(os.path.join(D.GOLDEN, f)) for f in files) < 300 * 1024
    for name, case in D.CASES.items():
        g = _golden(name)
        assert g["words"] == ["align"] + case["words"] and g["fail"] == case["fail"], name
    # the device ids of `GPU 3`, and --device
    assert [re.search(r"device=(\d+)", log).group(1) for _, log in sorted(_golden("box_3devices")["logs"].items(), key=lambda kv: int(kv[0]))] == ["0", "1", "2"]
    assert "device=1 " in _golden("box_device1")["logs"]["0"]
    # no statistics file for a run of no step
    assert _golden("stats_mean_steps0")["files"]["out_stats.nc"] is None and _golden("stats_mean")["files"]["out_stats.nc"]
    # a record assembled by 1, 2 or 3 slabs is the same bytes
    assert _golden("box")["files"] == _golden("box_2slabs")["files"] == _golden("box_3devices")["files"]
    for stat in ("stats_mean", "stats_variance", "stats_cov_every2"):
        assert _golden(stat)["files"] == _golden(stat + "_2slabs")["files"]


def test_every_refusal_of_the_driver_has_a_case():
    """Every std::runtime_error site of fs3d_run.cpp is reached by exactly one refusal case, or is listed with the reason why no command
    line reaches it: a refusal added without a case fails here."""
    def code(line):                                    # the line without its // comment (a // inside a string literal stays)
        for m in re.finditer("//", line):
            if line[:m.start()].count('"') % 2 == 0:
                return line[:m.start()]
        return line
    src = "\n".join(code(line) for line in open(D.DRIVER_SRC).read().splitlines())
    sites = [m.end() for m in re.finditer(r"std::runtime_error\(", src)]
    # what a site throws stands between it and the next site (the refusals follow one another), or within a few lines
    texts = [src[s:min(e, s + 600)] for s, e in zip(sites, sites[1:] + [len(src)])]
    owned = set()
    for frag in [frag for _, frag in D.REFUSALS.values()] + list(D.NOT_A_REFUSAL):
        hits = [i for i, text in enumerate(texts) if frag in text]
        assert len(hits) == 1 and hits[0] not in owned, (frag, hits)
        owned.add(hits[0])
    assert len(sites) == len(D.REFUSALS) + len(D.NOT_A_REFUSAL) and owned == set(range(len(sites))), [texts[i][:80] for i in set(range(len(sites))) - owned]


@pytest.mark.parametrize("name", D.TSAN_RUNS)
def test_slab_threads_are_race_free_under_thread_sanitizer(exe_tsan, name, tmp_path, monkeypatch):
    """The driver and the stand-in once more with -fsanitize=thread (a stand-alone program, nothing preloaded): the multi-slab moving
    and statistics runs return what the golden says and the sanitizer reports nothing (a report ends the run with exit code 66)."""
    monkeypatch.setenv("TSAN_OPTIONS", "halt_on_error=1:exitcode=66")
    got = D.run_case(exe_tsan, D.CASES[name], str(tmp_path / "run"))
    assert "ThreadSanitizer" not in got["stderr"], got["stderr"]
    _assert_equals_golden(got, _golden(name))
