"""csrc/ppcr_k1_plan.hpp — the one place that decides which K1 instantiation runs, on what grid, and what follows it —
as a stand-alone host program (tests/cpp/test_k1_plan.cc, plain g++): every query of its enumeration gives the plan that
launch_tile<M> chose by itself before the plan existed (tests/golden/k1_plan_table.txt.gz: recorded from that code with its
launch sites replaced by stand-ins that write down template arguments, grid and split table), and every plan keeps the
structural invariants the callers rely on.  No GPU."""
import gzip
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "probabilistic_point_clouds_registration_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")


def test_k1_plan_equals_the_recorded_decisions_and_keeps_its_invariants(tmp_path):
    exe = str(tmp_path / "k1_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_k1_plan.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    got = r.stdout.splitlines()
    assert got and got[-1].startswith("k1 plan test:") and got[-1].endswith(" 0 failed"), (r.stdout[-3000:] + r.stderr[-1000:])
    assert r.returncode == 0
    with gzip.open(os.path.join(ROOT, "tests", "golden", "k1_plan_table.txt.gz"), "rt") as f:
        want = f.read().splitlines()
    assert len(want) > 200000
    assert len(got) - 1 == len(want)
    for g, w in zip(got, want):
        assert g == w
