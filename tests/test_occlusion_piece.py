"""The piece planner of rptgpu_occluded and rptgpu_bake_ao (rpt_amd/csrc/render_plan.h occlusion_piece, ao_piece,
ao_pass_samples), compiled with g++ under AddressSanitizer and UBSan next to a driver that pins it
(tests/cpp/occlusion_piece_check.cpp): the pieces cover [0, n) once and in order, a piece of points never splits a point,
no pass exceeds its bound — for n = 0, n = 1 and for more samples per point than a pass holds."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("occlusion_piece") / "occlusion_piece_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "occlusion_piece_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("section", ["sizes", "cover", "ao", "planned"])
def test_occlusion_piece(checker, section):
    r = subprocess.run([checker, section], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and not r.stderr, r.stdout + r.stderr
