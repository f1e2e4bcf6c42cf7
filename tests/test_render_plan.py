"""The render planner (rpt_amd/csrc/render_plan.h), checked without a GPU: how a persistent batch is split into launches and
work items, and how the wavefront pipeline sizes its passes, retries them and measures record columns — compiled with
g++ and no ROCm include path next to a driver that pins literal values (tests/cpp/render_plan_check.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("render_plan") / "render_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "render_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["launches", "chunk", "items", "ratio", "passes", "retries", "bytes"])
def test_render_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
