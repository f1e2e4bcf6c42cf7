"""The scene planner (rpt_amd/csrc/scene_plan.h), checked without a GPU: the route of every top-level object, the re-route
after a live rebuild and the flat path kernel's LDS layout — compiled with g++ and no ROCm include path next to a driver
that carries the expressions scene creation held before the planner existed and compares field for field over the
boundaries of every rule, plus a few layouts derived by hand (tests/cpp/scene_plan_check.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_plan") / "scene_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "cpp", "scene_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["routing", "rerouting", "planes", "fits", "lights", "filter", "literal"])
def test_scene_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
