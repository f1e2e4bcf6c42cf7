"""Batches of interleaved IEEE f64 divisions (kernels/vec.inc div_ieee, RPT_DIV_BATCH) on a real MI355X.  A batch performs,
per slot, the eleven operations the compiler emits for `/` on the same operands, so nothing but the instruction order
changes: (1) the primitive, through rptgpu_eval_math's functions 8-11 (batches of 2, 3, 4 and 6 whose slots come from
different places of the operand arrays), equals numpy's `/` bit for bit over normal, huge, tiny, denormal, zero, infinite
and NaN operands; (2) the
frames and ray counts of the kernels equal those of a library built with -DRPT_DIV_BATCH=0 (scripts/build_variant.sh div0 "-DRPT_DIV_BATCH=0"), when there is one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import small_scenes  # noqa: E402
from rpt_amd import GpuScene, _abi, make_params, scenes  # noqa: E402

gpu = pytest.mark.gpu

AB_LIB = os.path.join(ROOT, "rpt_amd", "lib", "librptgpu_div0.so")  # scripts/build_variant.sh div0 "-DRPT_DIV_BATCH=0"
PERSISTENT = _abi.RPT_FLAG_PERSISTENT
FN_OF_WIDTH = {2: 8, 3: 9, 4: 10, 6: 11}
PAIRS = 1 << 20

_cases = []


def operand_cases():
    """the case list of test_gpu_parity.py::test_shared_reciprocal_division_is_ieee at 2^20 pairs per case: (numerators,
    denominators), generated once"""
    if _cases:
        return _cases
    rs = np.random.RandomState(17)
    n = PAIRS

    def rand_exp(lo, hi, size):
        m = rs.uniform(1.0, 2.0, size) * rs.choice([-1.0, 1.0], size)
        return np.ldexp(m, rs.randint(lo, hi, size))

    _cases.extend([
        (rs.randn(n), rs.randn(n)),
        (rs.uniform(-600, 600, n), rs.uniform(-1, 1, n)),
        (rand_exp(-450, 450, n), rand_exp(-450, 450, n)),
        (rand_exp(-1070, 1023, n), rand_exp(-1070, 1023, n)),  # denormals, overflow, underflow
        (rs.randint(-3, 4, n).astype(float), rs.randint(-3, 4, n).astype(float)),  # zeros, exact cases
    ])
    special = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1.7976931348623157e308, 2.0 ** -400,
                        2.0 ** 400, 2.0 ** -401, 3.0])
    yy, xx = np.meshgrid(special, special)
    _cases.append((yy.ravel().copy(), xx.ravel().copy()))
    return _cases


@pytest.fixture(scope="module")
def handle():
    g = GpuScene(scenes.sphere_scene()[0], 0)
    yield g
    g.close()


@gpu
@pytest.mark.parametrize("width", sorted(FN_OF_WIDTH))
def test_batched_division_is_ieee(handle, width):
    with np.errstate(all="ignore"):
        for y, x in operand_cases():
            got = handle.eval_math(FN_OF_WIDTH[width], x, y)
            ref = y / x
            same = (got.view(np.int64) == ref.view(np.int64)) | (np.isnan(got) & np.isnan(ref))
            assert same.all(), (width, int((~same).sum()), y[~same][:4], x[~same][:4], got[~same][:4], ref[~same][:4])


# ---- the kernels: every frame against the library without the batches
# name -> (scene of small_scenes / "cornell", width, height, bounces, spp, seed, the instantiation its launch lines must name)
FRAMES = {
    "cornell_96x64": ("cornell", 96, 64, 8, 4, 301, "rpt_paths<KdFlat>"),
    "cornell_33x17": ("cornell", 33, 17, 2, 3, 302, "rpt_paths<KdFlat>"),  # a partial last wave, paths ending at the bounce limit
    # the smallest small_scenes entry that runs each of the other kinds of instantiation, at its fixture's parameters
    "KdLds": ("cylinder", None, None, None, None, None, "rpt_paths<KdLds>"),
    "KdFlatG": ("sphere", None, None, None, None, None, "rpt_paths<KdFlatG>"),
    "KdFlatF": ("basic", None, None, None, None, None, "rpt_paths<KdFlatF>"),
}
FUSED = "shadow and bounce rays in one query"


def frame_inputs(name):
    src, w, h, b, spp, seed, _ = FRAMES[name]
    scene, cam, p = small_scenes.small(src)
    if w is None:
        return scene, cam, make_params(p.width, p.height, p.max_bounces, p.iterations, p.exposure_value, p.seed, flags=PERSISTENT)
    return scene, cam, make_params(w, h, b, spp, seed=seed, flags=PERSISTENT)


def render_frames(path):
    """every frame of FRAMES and its ray counts into an .npz; the launch lines go to stderr, each frame's behind a line
    `frame <name>`"""
    out = {}
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    for name in FRAMES:
        scene, cam, p = frame_inputs(name)
        g = GpuScene(scene, 0)
        sys.stderr.write("frame %s\n" % name)
        sys.stderr.flush()
        g.reset_stats()
        out[name] = g.render_batch(cam, p)
        st = g.stats()
        out[name + "_rays"] = np.array([st.extend_rays, st.shadow_rays], dtype=np.uint64)
        g.close()
    np.savez(path, **out)


def render_in_child(path, lib=None):
    env = dict(os.environ)
    env.pop("RPTGPU_LIB", None)
    if lib:
        env["RPTGPU_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, cur = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("frame "):
            cur = ln.split()[1]
            lines[cur] = []
        elif cur and ln.startswith("rpt_paths<"):
            lines[cur].append(ln)
    return np.load(path), lines


@gpu
@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="no library built with -DRPT_DIV_BATCH=0 (scripts/build_variant.sh div0)")
def test_library_without_the_batches_gives_the_same_frames(tmp_path):
    new, new_lines = render_in_child(str(tmp_path / "new.npz"))
    old, old_lines = render_in_child(str(tmp_path / "old.npz"), AB_LIB)
    for name, spec in FRAMES.items():
        for lines in (new_lines, old_lines):  # the frame ran through the instantiation it stands for, in both libraries
            assert lines.get(name) and all(ln.startswith(spec[6]) for ln in lines[name]), (name, lines.get(name))
            if spec[0] == "cornell":
                assert all(FUSED in ln for ln in lines[name]), lines[name]
        a, b = new[name], old[name]
        assert a.shape == b.shape and (a != 0).any(), name
        assert (a.view(np.int64) == b.view(np.int64)).all(), (name, np.abs(a - b).max())
        assert tuple(new[name + "_rays"]) == tuple(old[name + "_rays"]), name


if __name__ == "__main__":
    render_frames(sys.argv[1])
