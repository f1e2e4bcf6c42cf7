"""The channel tables without a GPU (rpt_amd/csrc/channel_plan.h): the header and the seven tables written
with it — RptHitArrays, RptAovBuffers, RptVertexArrays (render_plan.h), RptSurfaceArrays, RptLookupArrays, RptVolumeArrays,
RptLightmapArrays (their planners) — in a stand-alone program (tests/cpp/channel_plan_check.cpp), plain and under
AddressSanitizer + UBSan: the staging offsets by hand, every channel subset's layout, and the null check's row and text."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("channel_plan_" + request.param) / "channel_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "channel_plan_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "nulls"])
def test_channel_plan(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
