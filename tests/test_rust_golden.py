"""HIP == oracle == Rust, the day the Rust program's frames exist.

`bash scripts/pin_oracle.sh` (any machine with cargo) renders the golden configurations with the PATCHED REFERENCE
(rust/rpt.patch: the oracle's Philox stream behind rand's own distributions) and stores them as
tests/golden/rust_<scene>.npz.  This file consumes them: the CPU suite holds the oracle to the Rust frames, the GPU suite
holds the HIP path to them (and to the oracle, bit for bit).  Until the fixtures are committed every test here SKIPS with
the reason "parity unpinned" — the state SURVEY §8c describes: this image has no Rust toolchain, so no output of the
reference itself has ever been compared.

Tolerance, stated: per channel |delta| <= 1e-9 * max(1, |x|) on >= 98 % of the pixels.  Not 100 %: Rust's exp / ln / atan /
sin_cos / acos / atan2 are the platform libm's, the oracle's and the kernels' are fdlibm restated as IEEE arithmetic
(include/rpt_math.h; <= 1 ulp apart on about a tenth of the arguments), and one differing ulp can re-roll a rejection
loop or a lobe choice of that sample.  The oracle's system-libm build (liboracle_sysm.so) is reported beside it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from rpt_amd import golden_scenes, make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MIN_CLOSE = 0.98
UNPINNED = ("parity unpinned: tests/golden/rust_%s.npz is absent — no output of the Rust reference has been compared yet; "
            "run `bash scripts/pin_oracle.sh` on a machine with cargo and commit the fixtures")


def fixture(name):
    path = os.path.join(GOLDEN, "rust_%s.npz" % name)
    if not os.path.exists(path):
        pytest.skip(UNPINNED % name)
    z = np.load(path)
    extra = {"triangles": z["triangles"]} if "triangles" in z.files else {}
    scene, cam = golden_scenes.build(name, **extra)
    p = make_params(int(z["width"]), int(z["height"]), int(z["max_bounces"]), int(z["iterations"]), seed=int(z["seed"]))
    return scene, cam, p, z["image"].reshape(-1, 3)


def close_share(img, ref):
    return float((np.abs(img - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))).all(axis=1).mean())


@pytest.mark.parametrize("name", golden_scenes.NAMES)
def test_oracle_reproduces_the_rust_frames(oracle, name):
    scene, cam, p, ref = fixture(name)
    img = oracle.OracleScene(scene).render(cam, p, threads=0)
    assert img.shape == ref.shape
    assert close_share(img, ref) >= MIN_CLOSE, "oracle vs Rust: %.3f %% of pixels within 1e-9" % (100 * close_share(img, ref))
    assert abs(img.mean() - ref.mean()) <= 5e-3 * abs(ref.mean())


@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_scenes.NAMES)
def test_hip_path_reproduces_the_rust_frames(oracle, name):
    from rpt_amd import GpuScene
    scene, cam, p, ref = fixture(name)
    gpu = GpuScene(scene, 0)
    img = gpu.render_batch(cam, p)
    gpu.close()
    assert (img == oracle.OracleScene(scene).render(cam, p, threads=0)).all()  # HIP == oracle, bit for bit
    assert close_share(img, ref) >= MIN_CLOSE, "HIP vs Rust: %.3f %% of pixels within 1e-9" % (100 * close_share(img, ref))


def test_the_pinning_tools_work_end_to_end_on_a_stand_in_dump(oracle, tmp_path):
    """The plumbing of scripts/compare_rust_golden.py, exercised WITHOUT Rust: frames the oracle itself rendered are written
    in dump_golden.rs's file format and compared — this proves nothing about parity (the oracle agrees with itself), only
    that the day a real dump exists the tool reads it, compares, and says PASS / FAIL.  The teapot scene needs the crate's
    examples/teapot.obj: unpacked from tests/golden/assets into a stand-in crate directory."""
    import lzma
    d = tmp_path / "golden"
    d.mkdir()
    rpt_root = str(tmp_path / "rpt")
    os.makedirs(os.path.join(rpt_root, "examples"))
    with lzma.open(os.path.join(GOLDEN, "assets", "teapot.obj.xz")) as f, open(os.path.join(rpt_root, "examples", "teapot.obj"), "wb") as g:
        g.write(f.read())
    cfg = {"sphere": (64, 36, 2, 8, 101), "cornell": (64, 36, 8, 8, 102), "teapot": (64, 64, 6, 8, 103)}
    for name, (w, h, b, n, seed) in cfg.items():
        extra = {}
        if name == "teapot":
            from rpt_amd import io as rio
            extra["triangles"] = rio.load_obj(os.path.join(rpt_root, "examples", "teapot.obj")).triangles
            assert extra["triangles"].shape == (2256, 18)
        scene, cam = golden_scenes.build(name, **extra)
        img = oracle.OracleScene(scene).render(cam, make_params(w, h, b, n, seed=seed), threads=0)
        assert np.isfinite(img).all() and img.max() > 0
        img.astype("<f8").tofile(str(d / (name + ".f64")))
        (d / (name + ".txt")).write_text("width %d\nheight %d\nmax_bounces %d\niterations %d\nseed %d\n" % (w, h, b, n, seed))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "compare_rust_golden.py"), str(d), "--rpt-root", rpt_root]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("pin_oracle: PASS"), r.stdout[-800:] + r.stderr[-800:]
    # a frame that is NOT the oracle's must fail, loudly
    bad = np.fromfile(str(d / "sphere.f64"), dtype="<f8")
    (bad * 1.01).tofile(str(d / "sphere.f64"))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout.strip().splitlines()[-1].startswith("pin_oracle: FAIL"), r.stdout[-800:]


def test_pin_oracle_script_says_fail_without_cargo():
    import shutil
    if shutil.which("cargo"):
        pytest.skip("cargo present: run scripts/pin_oracle.sh itself")
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "pin_oracle.sh")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and r.stdout.strip().splitlines()[-1].startswith("pin_oracle: FAIL (cargo not found")
