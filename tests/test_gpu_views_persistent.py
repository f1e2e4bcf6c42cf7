"""RPT_FLAG_VIEWS_PERSISTENT on the GPU (include/rpt_gpu_views_persistent.h): a batch of views in the
persistent path kernel, rpt_paths_views.  Tolerance 0 (== on the f64 arrays) everywhere: the flagged call gives the frames
of the unflagged call of the same arguments — the wavefront pipeline's —, and a perspective view those of
rptgpu_render_batch of its camera and seed.

The scenes, and the instantiation each reaches (RPTGPU_PRINT_LAUNCH, `rpt_paths_views<...>: ...`, read once on an MI355X):
  cornell     37x21   rpt_paths_views<KdFlat>, shadow and bounce rays in one query, a hit's scene constants from the wave's
                      tables, pre-traced hits in a wave-level pool (the fused form with constants: POOL)
  glass       33x23   rpt_paths_views<KdFlatG> + parked environment lookups (the plain fetch, PARK)
  wine_glass  37x21   rpt_paths_views<KdLds> (deep trees: the general form)
  KdFlatG     64x48   rpt_paths_views<KdFlatG>: tests/test_gpu_parity.py's three spheres under a colour environment
  KdFlatF     64x48   rpt_paths_views<KdFlatF>: its polygon room behind the object filter
Sizes: tests/test_gpu_views.py's (more than one 256-thread block and an odd number of them) and test_gpu_parity.py's."""
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import Camera, GpuScene, Material, Object, View, _abi, cube, hex_color, make_params, scenes

import small_scenes
import test_gpu_parity as GP
import test_gpu_views as GV

pytestmark = pytest.mark.gpu

FLAG = _abi.RPT_FLAG_VIEWS_PERSISTENT
SPP, BASE = GV.SPP, GV.BASE
SMALL = ("cornell", "glass", "wine_glass")
NAMES = SMALL + ("KdFlatG", "KdFlatF")
SCATTERED = (0x52505447, 5, (1 << 63) + 1, 5)  # one seed per view of mixed()'s four: two of them equal, one past 2^63
WAVEFRONT_KINDS = (_abi.RPT_K_RAYGEN, _abi.RPT_K_EXTEND, _abi.RPT_K_SHADE, _abi.RPT_K_SHADOW, _abi.RPT_K_RESOLVE)


@functools.lru_cache(maxsize=None)
def setup(name):
    """-> (scene, (lens, orthographic, panorama, beside) — mixed()'s set —, width, height, max_bounces, seed)"""
    if name in SMALL:
        scene, _, p0 = small_scenes.small(name)
        plain, beside, lens, L = GV.cameras(name)
        w, h = GV.SIZES[name]
        return scene, (lens,) + GV.other_views(name) + (beside,), w, h, p0.max_bounces, p0.seed
    scene, lens = GP._thin_lens_scene(name)
    eye, direction, up = (np.array([float(c) for c in x]) for x in (lens.eye, lens.direction, lens.up))
    L = float(np.linalg.norm(eye))
    plain = Camera(lens.eye, lens.direction, lens.up, lens.fov, 0.0, 0.0)
    beside = Camera.look_at(tuple(eye + 0.15 * L * np.cross(direction, up) + 0.1 * L * up), tuple(eye + direction * L), tuple(up),
                            0.8 * lens.fov)
    views = (lens, View.orthographic(plain, L * math.tan(plain.fov / 2.0)), View.panorama(tuple(eye + 0.6 * L * direction)), beside)
    return scene, views, 64, 48, 3, 131


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GV.gpu(name) if name in SMALL else GpuScene(setup(name)[0], 0)


def render(g, name, views=None, **kw):
    _, all_views, w, h, bounces, seed = setup(name)
    kw.setdefault("samples", SPP)
    kw.setdefault("seed", seed)
    kw.setdefault("sample_index_base", BASE)
    return g.render_views(all_views if views is None else views, w, h, kw.pop("max_bounces", bounces), **kw)


def flagged(g, name, views=None, min_launches=1, **kw):
    """the call under RPT_FLAG_VIEWS_PERSISTENT, and RptStats as for a render through rpt_paths: the samples, the kernel's
    launches and rays — and no launch of a wavefront kind"""
    _, all_views, w, h, _, _ = setup(name)
    n = len(all_views if views is None else views)
    g.reset_stats()
    out = render(g, name, views, flags=FLAG | kw.pop("flags", 0), **kw)
    st = g.stats()
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= min_launches, "the persistent kernel did not run"
    assert [st.kernel_launches[k] for k in WAVEFRONT_KINDS] == [0] * len(WAVEFRONT_KINDS)
    assert st.samples == n * w * h * kw.get("samples", SPP)
    assert st.extend_rays >= st.samples
    return out


@functools.lru_cache(maxsize=None)
def reference(name, seeding):
    """the unflagged call's frames — seeding: a seed stride, or "seeds" for SCATTERED —, computed once, never written to"""
    if name in SMALL and seeding != "seeds":
        return GV.mixed(name, seeding)[1]
    kw = dict(seeds=SCATTERED) if seeding == "seeds" else dict(seed_stride=seeding)
    out = render(gpu(name), name, **kw)
    out.setflags(write=False)
    return out


def seed_kw(seeding):
    return dict(seeds=SCATTERED) if seeding == "seeds" else dict(seed_stride=seeding)


def test_the_library_reads_the_flag():
    assert _abi.views_persistent_supported()


@pytest.mark.parametrize("seeding", [0, 7, "seeds"], ids=["stride0", "stride7", "seeds"])
@pytest.mark.parametrize("name", NAMES)
def test_flagged_is_unflagged(name, seeding):
    """lens, orthographic, panorama, second perspective; 3 spp from sample 5: the flagged call == the unflagged one, and
    each perspective view == rptgpu_render_batch of its camera and seed"""
    _, views, w, h, bounces, seed = setup(name)
    g = gpu(name)
    want = reference(name, seeding)
    got = flagged(g, name, **seed_kw(seeding))
    assert got.shape == (4, h, w, 3) and got.dtype == np.float64 and np.isfinite(got).all()
    assert (got == want).all(), [int((got[v] != want[v]).any(axis=-1).sum()) for v in range(4)]
    for v in (0, 3):
        s = SCATTERED[v] if seeding == "seeds" else seed + v * seeding
        frame = g.render_batch(views[v], make_params(w, h, bounces, SPP, seed=s, sample_index_base=BASE))
        assert (got[v].reshape(-1, 3) == frame).all(), v
    assert not (got[0] == got[3]).all() and not (got[1] == got[2]).all()


@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("chunk", [1, 2])
@pytest.mark.parametrize("name", ["cornell", "KdFlatG"])
def test_a_wave_spans_views(name, chunk, stride):
    """5 views of 7x5: 35 pixels, so a wave's first claim holds pixels of two or three views, and 175 indices make a partial
    last wave; work items of 1 and 2 samples of 3"""
    scene, views, _, _, bounces, seed = setup(name)
    views = views + (views[0],)
    g = GpuScene(scene, 0, paths_chunk=chunk)
    try:
        kw = dict(samples=SPP, seed=seed, seed_stride=stride, sample_index_base=BASE)
        want = g.render_views(views, 7, 5, bounces, **kw)
        g.reset_stats()
        got = g.render_views(views, 7, 5, bounces, flags=FLAG, **kw)
        st = g.stats()
    finally:
        g.close()
    assert st.kernel_launches[_abi.RPT_K_PATHS] >= 1 and st.kernel_launches[_abi.RPT_K_RAYGEN] == 0
    assert st.samples == 5 * 35 * SPP
    assert (got == want).all() and np.isfinite(got).all()
    assert (got[4] == got[0]).all() == (stride == 0)  # the same view twice: the same frame under the same seed only


@pytest.mark.parametrize("stride", [0, 7])
@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_a_views_pixels_are_its_own(name, stride, monkeypatch):
    _, views, w, h, _, seed = setup(name)
    g = gpu(name)
    want = reference(name, stride)
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "100")  # pieces end inside views and span them
    assert (flagged(g, name, seed_stride=stride, min_launches=(4 * w * h + 99) // 100) == want).all()
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    # the views reversed, each with the seed it had
    seeds = [(seed + v * stride) % (1 << 64) for v in range(4)]
    assert (flagged(g, name, views[::-1], seeds=seeds[::-1]) == want[::-1]).all()
    for v in range(4):  # each view alone
        assert (flagged(g, name, views[v:v + 1], seed=seeds[v])[0] == want[v]).all(), v


def test_several_launches_per_piece():
    """a per-sample radiance buffer with room for ONE sample of the piece: three launches, fr.sample_base stepping"""
    scene, views, w, h, bounces, seed = setup("cornell")
    g = GpuScene(scene, 0, lbuf_bytes=4 * w * h * 24)
    try:
        g.reset_stats()
        got = g.render_views(views, w, h, bounces, samples=SPP, seed=seed, seed_stride=7, sample_index_base=BASE, flags=FLAG)
        launches = g.stats().kernel_launches[_abi.RPT_K_PATHS]
    finally:
        g.close()
    assert launches >= 3
    assert (got == reference("cornell", 7)).all()


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_sample_base_across_the_32_bit_boundary(name):
    g = gpu(name)
    kw = dict(seed_stride=7, sample_index_base=2 ** 32 - 2)
    want = render(g, name, **kw)
    assert (flagged(g, name, **kw) == want).all()
    assert not (want == reference(name, 7)).all()


@pytest.mark.parametrize("bounces", [0, None], ids=["0", "own"])
@pytest.mark.parametrize("name", ["cornell", "glass", "KdFlatF"])
def test_bounces(name, bounces):
    g = gpu(name)
    kw = dict(seed_stride=7) if bounces is None else dict(seed_stride=7, max_bounces=bounces)
    want = reference(name, 7) if bounces is None else render(g, name, **kw)
    assert (flagged(g, name, **kw) == want).all()


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_device_entry_point_into_torch_tensors(name):
    _, views, w, h, _, _ = setup(name)
    g = gpu(name)
    host = flagged(g, name, seed_stride=7)
    assert (host == reference(name, 7)).all()
    f64 = torch.full((4, h, w, 3), 7.0, dtype=torch.float64, device="cuda:0")
    assert flagged(g, name, seed_stride=7, out=f64) is f64
    assert (f64.cpu().numpy() == host).all()
    f32 = torch.full((4, h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
    flagged(g, name, seeds=[(setup(name)[5] + 7 * v) for v in range(4)], out=f32)
    assert (f32.cpu().numpy() == host.astype(np.float32)).all()


def test_after_a_live_update():
    """set_objects on the Cornell box: the flagged call on the updated handle == the flagged call on a fresh handle"""
    _, views, w, h, bounces, seed = setup("cornell")

    def moved():
        scene, _, _ = scenes.cornell()
        scene.objects[6] = Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
            .material(Material.diffuse(hex_color(0x3366CC)))
        return scene
    kw = dict(samples=SPP, seed=seed, seed_stride=7, sample_index_base=BASE, flags=FLAG)
    g = GpuScene(scenes.cornell()[0], 0)
    fresh = GpuScene(moved(), 0)
    try:
        before = g.render_views(views, w, h, bounces, **kw)
        g.set_objects([6], [moved().objects[6]])
        g.reset_stats()
        got = g.render_views(views, w, h, bounces, **kw)
        assert g.stats().kernel_launches[_abi.RPT_K_PATHS] >= 1 and g.stats().kernel_launches[_abi.RPT_K_RAYGEN] == 0
        want = fresh.render_views(views, w, h, bounces, **kw)
    finally:
        g.close()
        fresh.close()
    assert (got == want).all()
    assert (before == reference("cornell", 7)).all() and not (got == before).all()
