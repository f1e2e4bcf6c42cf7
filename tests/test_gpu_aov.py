"""First-hit feature buffers (rptgpu_render_aov) on a real MI355X against the oracle model of
tests/aov_model.py.  Every comparison is on the raw bits (f64 viewed as uint64), over every pixel, nothing excluded."""
import ctypes as C
import math

import numpy as np
import pytest

import rpt_amd
from rpt_amd import GpuScene, Material, Object, Renderer, _abi, cube, hex_color, make_params, scenes

import aov_model as M
import small_scenes

pytestmark = pytest.mark.gpu

ALL = _abi.RPT_AOV_ALL
FLAGS = {"persistent": _abi.RPT_FLAG_PERSISTENT, "wavefront": _abi.RPT_FLAG_WAVEFRONT,
         "general": _abi.RPT_FLAG_GENERAL_TRAVERSAL}
BITS = {"depth": 1, "normal": 2, "albedo": 4, "position": 8, "object": 16}


def with_(p, **kw):
    """a copy of RptRenderParams p with fields changed"""
    q = _abi.RptRenderParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def report(got, want, what):
    bad = M.mismatches(got, want)
    for name in bad:
        a, b = got[name], want[name]
        diff = (M.bits(a) != M.bits(b)) if a.dtype == np.float64 else (a != b)
        print("%s: %s differs in %d of %d elements" % (what, name, int(diff.sum()), diff.size))
    return bad


@pytest.mark.parametrize("name", small_scenes.NAMES)
def test_small_scenes_equal_the_model(name):
    scene, camera, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    got = g.render_aov(camera, p)
    g.close()
    want = M.full_frame(M.expected(scene, camera, p), p)
    assert got["hits"].sum() > 0
    assert report(got, want, name) == []


@pytest.mark.parametrize("name", ["cornell", "coverage", "wine_glass", "fractal_teapots", "seven_nest"])
def test_every_route_gives_the_default_routes_bits(name):
    scene, camera, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    base = g.render_aov(camera, p)
    for mode, flag in sorted(FLAGS.items()):
        got = g.render_aov(camera, with_(p, flags=flag))
        assert report(got, base, "%s under %s" % (name, mode)) == []
    again = g.render_aov(camera, p)  # (and the flags leave nothing behind in the handle)
    assert report(again, base, name + " again") == []
    g.close()


def test_pass_size_does_not_change_the_order_of_the_fold():
    scene, camera, p = small_scenes.small("wine_glass")
    p = with_(p, iterations=8)
    total = p.width * p.height * p.iterations
    n = 4608  # 2 samples per pixel per pass: four passes
    assert 1024 <= n < total / 3
    g = GpuScene(scene, 0)
    base = g.render_aov(camera, p)
    g.close()
    for flags in (0, _abi.RPT_FLAG_WAVEFRONT):
        g = GpuScene(scene, 0, target_paths=n)
        got = g.render_aov(camera, with_(p, flags=flags))
        g.close()
        assert report(got, base, "target_paths=%d flags=%d" % (n, flags)) == []
    assert base["hits"].max() == 8


@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_a_single_sample_is_the_closest_hit_itself(name):
    """iterations = 1: every sum is +0.0 + value (the value itself; a -0.0 comes out as +0.0, as the contract's sum
    does), and value is what rptgpu_closest_hit returns for the model's ray."""
    scene, camera, p = small_scenes.small(name)
    p = with_(p, iterations=1)
    exp = M.expected(scene, camera, p)
    o, d = exp["rays"]
    g = GpuScene(scene, 0)
    got = g.render_aov(camera, p)
    t, nrm, obj = g.closest_hit(o.reshape(-1, 3), d.reshape(-1, 3))
    g.close()
    h, w = p.height, p.width
    hit = obj >= 0
    assert hit.any()
    assert np.array_equal(got["object"].reshape(-1), obj)
    assert np.array_equal(got["hits"].reshape(-1), hit.astype(np.uint32))
    assert np.array_equal(M.bits(got["depth"].reshape(-1)), M.bits(np.where(hit, 0.0 + t, 0.0)))
    assert np.array_equal(M.bits(got["normal"].reshape(-1, 3)), M.bits(np.where(hit[:, None], 0.0 + nrm, 0.0)))


def test_parts_are_disjoint_and_sum_to_the_frame():
    scene, camera, p = small_scenes.small("coverage")
    g = GpuScene(scene, 0)
    full = g.render_aov(camera, p)
    parts = [g.render_aov(camera, with_(p, part_index=k, part_count=3)) for k in range(3)]
    g.close()
    owned = [M.owned(with_(p, part_index=k, part_count=3)) for k in range(3)]
    assert (sum(o.astype(int) for o in owned) == 1).all()
    for k, part in enumerate(parts):
        out = ~owned[k]
        assert (part["hits"][out] == 0).all() and (part["object"][out] == -1).all()
        for name in M.CHANNELS:
            assert (M.bits(part[name][out]) == 0).all(), (k, name)  # +0.0, not -0.0
        assert part["hits"][owned[k]].sum() > 0
    total = {"hits": sum(q["hits"] for q in parts), "object": np.maximum.reduce([q["object"] for q in parts])}
    for name in M.CHANNELS:
        total[name] = parts[0][name] + parts[1][name] + parts[2][name]
    assert report(total, full, "sum of the parts") == []


def _raw_call(g, camera, p, channels, sentinel=7):
    n = p.width * p.height
    keep = {"hits": np.full(n, sentinel, dtype=np.uint32), "depth": np.full(n, float(sentinel)),
            "normal": np.full((n, 3), float(sentinel)), "albedo": np.full((n, 3), float(sentinel)),
            "position": np.full((n, 3), float(sentinel)), "object": np.full(n, sentinel, dtype=np.int32)}
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = C.sizeof(b), channels
    types = dict(_abi.RptAovBuffers._fields_)
    for name, a in keep.items():
        setattr(b, name, a.ctypes.data_as(types[name]))
    cam = camera.lower()
    _abi.check(g.lib.rptgpu_render_aov(g.handle, C.byref(cam), C.byref(p), C.byref(b)), g.handle)
    return keep


@pytest.mark.parametrize("name", ["coverage", "wine_glass"])
def test_channel_mask(name):
    scene, camera, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    full = _raw_call(g, camera, p, ALL)
    for ch, bit in BITS.items():
        one = _raw_call(g, camera, p, bit)
        assert np.array_equal(one["hits"], full["hits"])
        for other in BITS:
            a = one[other]
            if other == ch:
                same = np.array_equal(M.bits(a), M.bits(full[other])) if a.dtype == np.float64 else np.array_equal(a, full[other])
                assert same, (ch, other)
            else:
                assert (a == 7).all(), "%s alone wrote into %s" % (ch, other)
    none = _raw_call(g, camera, p, 0)
    assert np.array_equal(none["hits"], full["hits"]) and all((none[k] == 7).all() for k in BITS)
    got = g.render_aov(camera, p, channels=_abi.RPT_AOV_DEPTH | _abi.RPT_AOV_NORMAL)
    assert sorted(got) == ["depth", "hits", "normal"]
    g.close()


@pytest.mark.parametrize("name", ["coverage", "wine_glass"])
def test_sample_index_base(name):
    scene, camera, p = small_scenes.small(name)
    g = GpuScene(scene, 0)
    four = g.render_aov(camera, with_(p, iterations=4, sample_index_base=0))
    a = g.render_aov(camera, with_(p, iterations=2, sample_index_base=0))
    b = g.render_aov(camera, with_(p, iterations=2, sample_index_base=2))
    g.close()
    assert np.array_equal(a["hits"] + b["hits"], four["hits"])
    assert np.array_equal(a["object"], four["object"])
    want_b = M.full_frame(M.expected(scene, camera, with_(p, iterations=2, sample_index_base=2)), p)
    assert report(b, want_b, "base 2") == []  # (object of the second call is sample 2's)
    one = M.full_frame(M.expected(scene, camera, with_(p, iterations=1, sample_index_base=2)), p)
    assert np.array_equal(b["object"], one["object"])
    assert not np.array_equal(M.bits(a["depth"]), M.bits(b["depth"]))


def test_live_update_equals_a_fresh_handle():
    scene, camera, p = small_scenes.small("cornell")
    g = GpuScene(scene, 0)
    before = g.render_aov(camera, p)
    moved, _, _ = scenes.cornell()
    moved.objects[6] = Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
        .material(Material.diffuse(hex_color(0x3366CC)))
    g.set_objects([6], [moved.objects[6]])
    for flags in (0, _abi.RPT_FLAG_WAVEFRONT):
        got = g.render_aov(camera, with_(p, flags=flags))
        f = GpuScene(moved, 0)
        want = f.render_aov(camera, with_(p, flags=flags))
        f.close()
        assert report(got, want, "after set_objects, flags=%d" % flags) == []
    assert report(got, M.full_frame(M.expected(moved, camera, p), p), "updated scene against the model") == []
    assert not np.array_equal(M.bits(got["albedo"]), M.bits(before["albedo"]))
    assert not np.array_equal(M.bits(got["depth"]), M.bits(before["depth"]))
    g.close()


def _probe_pixels(w, h, tile=(32, 8), count=20000, seed=0xA0F):
    """a seeded random set of `count` pixels, the four corners, and the pixels on both sides of the first and the last
    tile edge in x and in y (whole columns and rows)"""
    rng = np.random.default_rng(seed)
    pix = {(int(x), int(y)) for x, y in zip(rng.integers(0, w, count), rng.integers(0, h, count))}
    pix |= {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}
    tw, th = tile
    last_x, last_y = (w - 1) // tw * tw, (h - 1) // th * th
    for ex in (tw, last_x):
        for x in (ex - 1, ex):
            pix |= {(x, y) for y in range(h)}
    for ey in (th, last_y):
        for y in (ey - 1, ey):
            pix |= {(x, y) for x in range(w)}
    return sorted(pix, key=lambda q: (q[1], q[0]))


@pytest.mark.parametrize("config", ["C2", "C5"])
def test_full_frame_against_the_model(config):
    if config == "C2":
        scene, camera, _ = scenes.cornell()
        p = make_params(1920, 1080, 8, 2, seed=0xC2)
    else:
        scene, camera, _ = scenes.wine_glass()
        p = make_params(3840, 2160, 16, 1, seed=0xC5)
    g = GpuScene(scene, 0)
    got = g.render_aov(camera, p)
    g.close()
    pixels = _probe_pixels(p.width, p.height)
    assert len(pixels) >= 20000
    exp = M.expected(scene, camera, p, pixels)
    xs = np.array([q[0] for q in pixels])
    ys = np.array([q[1] for q in pixels])
    sub = {name: got[name][ys, xs] for name in ("hits", "object") + M.CHANNELS}
    assert exp["hits"].sum() > 0
    assert report(sub, exp, config) == []


def test_renderer_render_aovs_gives_means():
    scene, camera, p = small_scenes.small("sphere")
    r = Renderer(scene, camera).width(p.width).height(p.height).num_samples(p.iterations).seed(p.seed)
    means = r.render_aovs()
    sums = r.gpu_scene().render_aov(camera, with_(p, sample_index_base=0))
    hits = sums["hits"]
    assert np.array_equal(means["hits"], hits) and np.array_equal(means["object"], sums["object"])
    hit = hits > 0
    assert hit.any()
    for name in M.CHANNELS:
        n = hits[hit].astype(np.float64)
        want = sums[name][hit] / (n if sums[name].ndim == 2 else n[:, None])
        assert np.array_equal(M.bits(means[name][hit]), M.bits(want)), name
        assert (M.bits(means[name][~hit]) == 0).all() and np.isfinite(means[name]).all(), name
    # a frame with misses: the unit sphere alone, seen from afar
    lone = rpt_amd.Scene()
    lone.add(Object(rpt_amd.sphere()))
    cam = rpt_amd.Camera.look_at((0.0, 0.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), math.pi / 4)
    m = Renderer(lone, cam).width(48).height(32).num_samples(3).render_aovs()
    miss = m["hits"] == 0
    assert miss.any() and (~miss).any()
    for name in M.CHANNELS:
        assert (M.bits(m[name][miss]) == 0).all() and np.isfinite(m[name]).all()
    assert (m["object"][miss] == -1).all() and (m["object"][m["hits"] == 3] == 0).all()
