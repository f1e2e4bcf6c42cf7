"""The index arithmetic of rpt_paths' wave-level pool of pre-traced camera hits (rpt_amd/csrc/hit_pool.h, shared with the
kernel: kernels/paths.inc POOL), checked without a GPU by a host program that keeps a model of what every slot holds
(tests/cpp/hit_pool_check.cpp), compiled with g++ and no ROCm include path.

fifo    exhaustive over head, count, pop mask size and push mask size (several lane placements each) for capacities 1..9:
        no slot is overwritten before it is popped, rank r of a pop takes the r-th oldest entry, 0 <= count <= capacity
stream  20 000 iterations of the kernel's loop (refill by the predicate, then pop) per pool shape, the shipped ones among them
refill  exhaustive for capacities 1..16: without a refill every lane that needs a hit finds one; with one, a lane goes
        without only if every cursor that has work generated in the pass (one sample per cursor and pass)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hit_pool") / "hit_pool_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "hit_pool_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["fifo", "stream", "refill"])
def test_hit_pool(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
