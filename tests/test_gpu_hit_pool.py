"""The wave-level pool of pre-traced camera hits of the fused path kernels (kernels/paths.inc POOL, RPT_HIT_POOL;
rpt_amd/csrc/hit_pool.h) on a real MI355X.  Which lane runs a sample changes nothing it computes, so every frame must equal
the oracle's BIT for bit, with the oracle's closest-hit and shadow ray counts, and the wavefront pipeline's frame and
counts, through the fused kernel with the pool (the launch diagnostics say so).  The shapes are the smallest at which the
pool can go wrong:

few_items    8x4 pixels, 1 spp: fewer items than lanes, half the cursors are exhausted from the start
item_ends    16x8 pixels, 17 spp: items end inside a refill, and the last item of a pixel is shorter than its chunk
ragged       33x7 pixels, 5 spp: ragged tiles
b0, b1       max_bounces 0 and 1: every lane pops in every (other) iteration, the pool starves and refills are forced
escape       the camera turned away from the room: most camera rays escape, so entries are escaped ones and a lane pops
             again in the next iteration (the oracle's counts at 0 bounces say how many escaped)
lens         a thin-lens camera: no screen rectangles, unit_disc's rejection loop runs in the refill
second call  the same handle again with another sample_index_base
partition    tile / part with few tiles per part
and the same frames from a library built with -DRPT_HIT_POOL=0, when there is one."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rpt_amd import Camera, GpuScene, _abi, make_params, scenes  # noqa: E402

gpu = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS
WAVEFRONT = _abi.RPT_FLAG_WAVEFRONT | _abi.RPT_FLAG_PROFILE_KERNELS
FUSED = "shadow and bounce rays in one query"
POOL = "pre-traced hits in a wave-level pool"
AB_LIB = os.path.join(ROOT, "rpt_amd", "lib", "librptgpu_pool0.so")  # scripts/build_variant.sh pool0 "-DRPT_HIT_POOL=0"


def camera(kind):
    _, cam, _ = scenes.cornell()
    if kind == "away":  # the room at the left edge of the frame: three camera rays in four miss it
        cam = Camera.look_at((278.0, 273.0, -800.0), (900.0, 400.0, 280.0), (0.0, 1.0, 0.0), 0.686)
    elif kind == "lens":
        cam = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
        cam.focus((278.0, 273.0, 280.0), 25.0)
        assert cam.aperture > 0.0
    return cam


# every frame the tests compare: name -> (camera, width, height, max_bounces, spp, further parameters)
CASES = {
    "few_items": ("shipped", 8, 4, 8, 1, {}),
    "item_ends": ("shipped", 16, 8, 8, 17, {}),
    "ragged": ("shipped", 33, 7, 8, 5, {}),
    "b0": ("shipped", 33, 7, 0, 5, {}),
    "b1": ("shipped", 16, 8, 1, 17, {}),
    "escape": ("away", 40, 24, 8, 6, {}),
    "escape_b0": ("away", 40, 24, 0, 6, {}),
    "lens": ("lens", 33, 7, 4, 5, {}),
    "lens_b0": ("lens", 16, 8, 0, 17, {}),
    "later_samples": ("shipped", 16, 8, 8, 17, {"sample_index_base": 17}),
    "part0": ("shipped", 33, 7, 8, 3, {"tile": (8, 4), "part": (0, 3)}),
    "part1": ("shipped", 33, 7, 8, 3, {"tile": (8, 4), "part": (1, 3)}),
    "part2": ("shipped", 33, 7, 8, 3, {"tile": (8, 4), "part": (2, 3)}),
}
_refs = {}


def params(name, flags=PERSISTENT):
    _, w, h, b, spp, kw = CASES[name]
    return make_params(w, h, b, spp, seed=37, flags=flags, **kw)


def reference(osc, name):
    """the oracle's frame and ray counts of a case, rendered once"""
    if name not in _refs:
        _refs[name] = osc.render(camera(CASES[name][0]), params(name), threads=0, counters=True)
    return _refs[name]


def assert_pool(g, cam, capfd):
    """the launch diagnostics (RPTGPU_PRINT_LAUNCH) of one small render name the fused kernel with the pool"""
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]
    assert lines and all(FUSED in ln and POOL in ln for ln in lines), lines


def check(g, osc, name):
    """the persistent pipeline's frame and counts against the oracle's, and the wavefront pipeline's against both"""
    cam = camera(CASES[name][0])
    ref, cnt = reference(osc, name)
    for flags in (PERSISTENT, WAVEFRONT):
        g.reset_stats()
        img = g.render_batch(cam, params(name, flags))
        st = g.stats()
        if flags == PERSISTENT:
            assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1  # the persistent kernel ran
        assert (img.view(np.int64) == ref.view(np.int64)).all(), (name, flags, np.abs(img - ref).max())
        assert st.extend_rays == cnt["closest_rays"], (name, flags, st.extend_rays, cnt["closest_rays"])
        assert st.shadow_rays == cnt["shadow_rays"], (name, flags, st.shadow_rays, cnt["shadow_rays"])
    return ref


@pytest.fixture(scope="module")
def c2(oracle):
    scene, _, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    yield g, oracle.OracleScene(scene)
    g.close()


@gpu
@pytest.mark.parametrize("name", ["few_items", "item_ends", "ragged"])
def test_items_and_cursors(c2, capfd, name):
    g, osc = c2
    assert_pool(g, camera("shipped"), capfd)
    img = check(g, osc, name)
    assert np.isfinite(img).all() and img.max() > 0.0


@gpu
@pytest.mark.parametrize("name", ["b0", "b1"])
def test_short_paths_starve_the_pool(c2, name):
    g, osc = c2
    check(g, osc, name)


@gpu
def test_most_camera_rays_escape(c2, capfd):
    g, osc = c2
    assert_pool(g, camera("away"), capfd)
    _, cnt = reference(osc, "escape_b0")  # at 0 bounces: one closest-hit ray per sample, one shadow ray per camera hit
    assert 0 < cnt["shadow_rays"] < 0.5 * cnt["closest_rays"], cnt
    check(g, osc, "escape_b0")
    check(g, osc, "escape")


@gpu
def test_lens_camera(c2, capfd):
    g, osc = c2
    assert_pool(g, camera("lens"), capfd)
    check(g, osc, "lens")
    check(g, osc, "lens_b0")


@gpu
def test_second_call_with_another_sample_base(c2):
    g, osc = c2
    first = check(g, osc, "item_ends")
    second = check(g, osc, "later_samples")
    assert not (first == second).all()
    assert (check(g, osc, "item_ends") == first).all()


@gpu
def test_partition_with_few_tiles(c2):
    g, osc = c2
    acc = None
    for i in range(3):
        img = check(g, osc, "part%d" % i)
        acc = img if acc is None else acc + img
    assert np.isfinite(acc).all() and acc.max() > 0.0


def render_cases(path):
    """(a process of its own, under RPTGPU_LIB) every case's frame and ray counts into an .npz; the launch lines go to stderr"""
    scene, _, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    out = {}
    for name in CASES:
        cam = camera(CASES[name][0])
        g.reset_stats()
        out[name] = g.render_batch(cam, params(name))
        st = g.stats()
        out[name + "_rays"] = np.array([st.extend_rays, st.shadow_rays], dtype=np.uint64)
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    g.render_batch(camera("shipped"), make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
    del os.environ["RPTGPU_PRINT_LAUNCH"]
    g.close()
    np.savez(path, **out)


@gpu
@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="no library built with -DRPT_HIT_POOL=0 (scripts/build_variant.sh pool0)")
def test_library_with_the_per_lane_stash_gives_the_same_frames(c2, tmp_path):
    g, osc = c2
    out = str(tmp_path / "frames.npz")
    env = dict(os.environ, RPTGPU_LIB=AB_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("rpt_paths<")]
    assert lines and all(FUSED in ln and POOL not in ln for ln in lines), lines
    got = np.load(out)
    for name in CASES:
        ref, cnt = reference(osc, name)
        img = g.render_batch(camera(CASES[name][0]), params(name))
        assert (got[name].view(np.int64) == img.view(np.int64)).all(), name
        assert (got[name].view(np.int64) == ref.view(np.int64)).all(), name
        assert tuple(int(v) for v in got[name + "_rays"]) == (cnt["closest_rays"], cnt["shadow_rays"]), name


if __name__ == "__main__":
    render_cases(sys.argv[1])
