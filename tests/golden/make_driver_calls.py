#!/usr/bin/env python3
"""Generates tests/golden/driver_calls/<case>.json: what host/fs3d_run.cpp does, call by call, for every command line of the matrix in
tests/driver_calls.py -- return code, stderr, stdout with the host-clock numbers masked, the call log of every context of the recording
stand-in (tests/fs3d_stub.cpp) and the sha256 of the result files.  tests/test_host_driver_calls.py holds the driver to them.
They were made from the driver as it stood BEFORE its two time loops became one, and are not made again when the driver changes: a
change of the driver that moves one of these files is a change of behaviour.  To reproduce them, put that commit's
cmc_fluid_solver_amd/host/fs3d_run.cpp into a copy of this tree and run there:  python tests/golden/make_driver_calls.py
Needs g++ only; no GPU, no libfs3d_hip.so.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import driver_calls as D

os.makedirs(D.GOLDEN, exist_ok=True)
total = 0
with tempfile.TemporaryDirectory() as tmp:
    exe = D.build(os.path.join(tmp, "bin"))
    for name, case in D.CASES.items():
        rec = D.run_case(exe, case, os.path.join(tmp, "run"))
        path = os.path.join(D.GOLDEN, name + ".json")
        with open(path, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        total += os.path.getsize(path)
        print("%-40s rc %3d, %d contexts, %6d bytes" % (name, rec["returncode"], len(rec["logs"]), os.path.getsize(path)))
print(len(D.CASES), "cases,", total, "bytes")
