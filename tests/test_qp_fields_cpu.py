"""csrc/qp_fields.h, the one table of the C-ABI's QP arrays: the stand-alone host program
build/qp_fields_test (csrc/test/qp_fields_test.cpp, built by `make all` with the address and
undefined-behaviour sanitizers) checks that every visitor reaches each pointer member of its
struct exactly once, that the per-QP counts equal literals, and the staging plan's layout."""
import subprocess

import helpers


def test_qp_fields_program():
    exe = helpers.REPO / "build" / "qp_fields_test"
    assert exe.exists(), f"{exe} is missing: run `make all` (or __graft_entry__.build())"
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qp_fields_test: ok" in r.stdout
