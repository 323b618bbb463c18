"""GPU: every filtered and derived result record of tests/output_digest_cases.py, bit for bit.  The digests of
tests/golden/output_record_digests.json were recorded with the library as it stood before k_get_layer_box and get_layer_impl
(csrc/kernels_output.hip) served the whole grid and the x-slabs alike; the fields are order-sensitive (test_output_digest_cases.py),
so a change in the order of any sum of the record path shows here, which the bounds of the other record tests let pass."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import output_digest_cases as DC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch_first():
    import torch
    torch.cuda.init()                    # before the library opens the device


@pytest.fixture(autouse=True)
def _exact_kernels(monkeypatch):
    monkeypatch.setenv("FS3D_DEFAULT_KERNEL", "4")


@pytest.fixture(scope="module")
def recorded():
    with open(DC.GOLDEN) as f:
        return json.load(f)


def test_every_recorded_digest_belongs_to_a_run(recorded):
    keys = [k for _, fn, args in DC.RUNS for k in _expected_keys(fn, args)]
    assert len(keys) == len(set(keys)) and set(keys) == set(recorded)


def _expected_keys(fn, args):
    if fn is DC.run_stats:
        return ["stats-whole-" + DC.name(args[0]), "stats-slabs-on-%d-%s" % (DC.STAT_RANKS, DC.name(args[0]))]
    base, dtype, dev = (DC.whole_id(*args[:2]), args[2], args[3]) if fn is DC.run_whole else (DC.slab_id(args[0]), args[1], args[2])
    return [DC.mode_key(base, dtype, f, v, e) for f, v in DC.MODES for e in (("host", "dev") if dev else ("host",))]


@pytest.mark.parametrize("fn,args", [r[1:] for r in DC.RUNS], ids=[r[0] for r in DC.RUNS])
def test_records_are_the_recorded_ones_bit_for_bit(built, recorded, fn, args):
    got = fn(*args)
    assert sorted(got) == sorted(_expected_keys(fn, args))
    wrong = [k for k in got if got[k] != recorded[k]]
    assert not wrong, wrong
