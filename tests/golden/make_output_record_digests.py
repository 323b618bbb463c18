#!/usr/bin/env python3
"""Generates tests/golden/output_record_digests.json: case id -> sha256 of the bytes of outV followed by outT, for every run of
tests/output_digest_cases.py.  tests/test_gpu_output_record_digests.py holds the tree's library to them.
They were recorded ONCE, with the library of the commit before the two box kernels and the two host bodies of the result records
became one (5de51b5, "Filtered and derived result records on x-slabs"), and are not made again when the output path changes: a
change there that moves one of these digests is a change of a record's bits.  To reproduce them, build that commit's library and run
    FS3D_LIB_PATH=<that libfs3d_hip.so> python tests/golden/make_output_record_digests.py [output file]
Needs the GPU."""
import json
import os
import sys

os.environ["FS3D_DEFAULT_KERNEL"] = "4"                    # the steps of the time-statistics case run on the bit-exact kernels
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import torch  # noqa: E402

torch.cuda.init()                                          # before the library opens the device
import output_digest_cases as DC  # noqa: E402

digests = {}
for rid, fn, args in DC.RUNS:
    got = fn(*args)
    assert not set(got) & set(digests)
    digests.update(got)
    print("%-60s %d records" % (rid, len(got)))
path = sys.argv[1] if len(sys.argv) > 1 else DC.GOLDEN
with open(path, "w") as f:
    json.dump(digests, f, indent=0, sort_keys=True)
    f.write("\n")
print(len(digests), "digests ->", path)
