"""The shadow ray's window in the two-ray query (RPT_SHADOW_WINDOW), checked without a GPU: tests/cpp/shadow_window_check.cpp
compiled with g++, -ffp-contract=off like the kernels, under AddressSanitizer and UBSan, and run on the CPU.  It holds the
rule's inequality (every time an axis-flat object's leaf can accept is >= max(q, EPSILON) * (1 - 2^-50), and the rule never drops
a hit at or before t_stop) over 1.2e7 seeded draws, and the host's derivation of the mark (scene_plan.h axis_flat_mesh, plan_flat)
on C2's walls and light and on every way a mesh can fail it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shadow_window_check(tmp_path):
    exe = str(tmp_path / "shadow_window_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "shadow_window_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[3]) >= 10_000_000 and int(r.stdout.split()[1]) > int(r.stdout.split()[3]) // 2
