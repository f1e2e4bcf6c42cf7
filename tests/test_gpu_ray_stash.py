"""rpt_paths<KdFlat, false> with pre-traced camera rays (kernels/paths.inc, RPT_RAY_STASH=2) on a real MI355X: a lane
whose ray escaped shades its stashed hit in the same iteration.  Every frame is compared BIT for bit with the oracle,
through the persistent kernel, at the histories the swap changes: bounce limits 0-8, sample counts that are not a
multiple of the work item's chunk, many pre-traced rays that escape, work that runs out while rays wait in the stash,
later sample batches and a tile partition.  The closest-hit ray count must equal the oracle's and the wavefront
pipeline's: every pre-traced ray is traced, and counted, once."""
import numpy as np
import pytest

from rpt_amd import Camera, GpuScene, _abi, make_params, scenes

pytestmark = pytest.mark.gpu

PERSISTENT = _abi.RPT_FLAG_PERSISTENT | _abi.RPT_FLAG_PROFILE_KERNELS


@pytest.fixture(scope="module")
def cornell(oracle):
    scene, cam, _ = scenes.cornell()
    g = GpuScene(scene, 0)
    g3 = GpuScene(scene, 0, paths_chunk=3)
    yield scene, cam, g, g3, oracle.OracleScene(scene)
    g.close()
    g3.close()


def params(w, h, b, spp, flags=PERSISTENT, **kw):
    return make_params(w, h, b, spp, seed=kw.pop("seed", 11), flags=flags, **kw)


def check(g, osc, cam, p):
    g.reset_stats()
    img = g.render_batch(cam, p)
    st = g.stats()
    ref, cnt = osc.render(cam, p, threads=0, counters=True)
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1  # the persistent kernel ran
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (p.width, p.height, p.max_bounces, np.abs(img - ref).max())
    assert st.extend_rays == cnt["closest_rays"], (st.extend_rays, cnt["closest_rays"])
    return img, st, cnt


@pytest.mark.parametrize("bounces", [0, 1, 2, 8])
def test_scaled_cornell_matches_the_oracle(cornell, bounces):
    scene, cam, g, _, osc = cornell
    check(g, osc, cam, params(320, 180, bounces, 16))  # more work items than lanes: the stash refills in steady state


def test_spp_not_a_multiple_of_the_chunk(cornell):
    scene, cam, _, g3, osc = cornell
    check(g3, osc, cam, params(160, 90, 8, 7))
    check(g3, osc, cam, params(96, 54, 3, 11, seed=5))


def test_camera_looking_mostly_past_the_box(cornell):
    scene, _, g, _, osc = cornell
    cam = Camera(eye=(278.0, 273.0, -800.0), direction=(0.6, 0.1, 0.8), up=(0.0, 1.0, 0.0), fov=0.686)
    _, _, cnt = check(g, osc, cam, params(240, 135, 8, 8))
    assert cnt["misses"] > 0.5 * cnt["samples"]  # most camera rays escape


def test_frame_smaller_than_the_grid(cornell):
    scene, cam, g, _, osc = cornell
    for w, h, spp in ((5, 3, 3), (17, 9, 2), (1, 1, 40)):
        check(g, osc, cam, params(w, h, 8, spp))


def test_later_sample_batches(cornell):
    scene, cam, g, _, osc = cornell
    check(g, osc, cam, params(96, 54, 8, 6, sample_index_base=6))
    check(g, osc, cam, params(64, 36, 4, 5, sample_index_base=2 ** 32 - 3))


def test_tile_partition(cornell):
    scene, cam, g, _, osc = cornell
    acc = None
    for i in range(4):
        img = check(g, osc, cam, params(128, 72, 8, 4, tile=(32, 8), part=(i, 4)))[0]
        acc = img if acc is None else acc + img
    whole = check(g, osc, cam, params(128, 72, 8, 4))[0]
    assert (acc == whole).all()


def test_ray_counts_equal_the_wavefront_pipelines(cornell):
    scene, cam, g, _, osc = cornell
    img, st, _ = check(g, osc, cam, params(320, 180, 8, 8))
    g.reset_stats()
    pw = params(320, 180, 8, 8, flags=_abi.RPT_FLAG_WAVEFRONT | _abi.RPT_FLAG_PROFILE_KERNELS)
    assert (g.render_batch(cam, pw) == img).all()
    st2 = g.stats()
    assert (st2.extend_rays, st2.shadow_rays, st2.samples) == (st.extend_rays, st.shadow_rays, st.samples)
