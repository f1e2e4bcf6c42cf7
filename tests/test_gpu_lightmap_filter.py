"""rptgpu_filter_lightmap on the GPU, held to include/rpt_gpu_lightmap_filter.h to the bit.

The call against tests/lightmap_filter_model.py, the header restated in numpy (itself held by hand in
tests/test_lightmap_filter_host.py), on synthetic maps — gutters and unowned islands, a crease, a step between parallel planes,
two coplanar charts adjacent in the atlas and far apart in the world, a NaN and an infinite value, a NaN normal, a NaN
position — at the sizes where the 64 x 4 blocks end, and on real bakes; levels == 0 against rptgpu_bake_lightmap's own
dilation; device tensors against host arrays; the arrays it must leave alone; its independence of the handle's scene.  Every
comparison is on the bits (lightmap_model.same)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi, lightmap

import lightmap_filter_model as F
import lightmap_model as M
import small_scenes
import surface_model

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SCENES = ["cornell", "wine_glass"]
SIG = dict(sigma_normal=0.1, sigma_plane=0.05, sigma_distance=0.4)
ALL = (_abi.RPT_LIGHTMAP_IRRADIANCE | _abi.RPT_LIGHTMAP_AO | _abi.RPT_LIGHTMAP_OWNER | _abi.RPT_LIGHTMAP_POSITION |
       _abi.RPT_LIGHTMAP_NORMAL)


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


# ---- synthetic maps
@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """-> owner, position, normal, values3, values1, variance (read-only).  Five bands of columns, texels of 0.1 world units:
    0 a floor y = 0; 1 a wall that meets it in a crease; 2 the floor again, 0.05 higher (a step between parallel planes, no
    gutter before it); 3 the floor's own plane 100 units away (coplanar, adjacent in the atlas, far apart in the world); 4 a
    tilted plane.  Every seventh column is a gutter and a lattice of single texels is unowned; their guides are +0.0 as a bake
    leaves them, their values are not.  Four valid texels, where the map has enough, hold a NaN value, an infinite value, a
    NaN normal and a NaN position."""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    band = (x * 5) // w
    u, z = 0.1 * (x + 0.5), 0.1 * (y + 0.5)
    zero = np.zeros((h, w))
    edge = 0.1 * (np.ceil(w / 5.0))                      # where band 1 begins, in the floor's x
    tilt = (0.0, np.cos(0.4), np.sin(0.4))
    position = np.select([(band == k)[..., None] for k in range(5)],
                         [np.stack([u, zero, z], axis=-1), np.stack([zero + edge, u - edge, z], axis=-1),
                          np.stack([u, zero + 0.05, z], axis=-1), np.stack([100.0 + u, zero, z], axis=-1),
                          np.stack([u, 0.2 + np.sin(0.4) * z, np.cos(0.4) * z], axis=-1)])
    normal = np.select([(band == k)[..., None] for k in range(5)],
                       [np.broadcast_to(n, (h, w, 3)) for n in ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), tilt)])
    owner = band.astype(np.int32)
    if w * h > 1:
        owner[(x % 7 == 3) | ((3 * x + 5 * y) % 11 == 0)] = -1
    valid = owner >= 0
    position[~valid], normal[~valid] = 0.0, 0.0
    values3 = 1.0 + 0.3 * np.sin(u + z)[..., None] * np.array([1.0, 0.5, 2.0]) + rng.normal(0.0, 0.2, size=(h, w, 3))
    values1 = 0.5 + 0.2 * np.cos(u - z) + rng.normal(0.0, 0.1, size=(h, w))
    variance = rng.uniform(0.001, 0.1, size=(h, w))
    where = np.argwhere(valid)
    if len(where) >= 16:
        picks = [tuple(where[(k * len(where)) // 5]) for k in (1, 2, 3, 4)]
        values3[picks[0]][1], values1[picks[0]] = NAN, NAN
        values3[picks[1]][2], values1[picks[1]] = INF, -INF
        normal[picks[2]] = (0.0, NAN, 0.0)
        position[picks[3]] = (NAN, 0.0, 0.0)
    out = (owner, position, normal, values3, values1, variance)
    for a in out:
        a.setflags(write=False)
    return out


# one block exactly, one past it in both directions, and steps beyond the map
SIZES = [(1, 1, 3), (13, 7, 3), (64, 4, 3), (65, 5, 3), (130, 9, 8)]


@pytest.mark.parametrize("with_variance", [False, True], ids=["plain", "variance"])
@pytest.mark.parametrize("words", [1, 3])
@pytest.mark.parametrize("w,h,levels", SIZES, ids=["%dx%d-%dlevels" % s for s in SIZES])
def test_the_call_is_the_models(w, h, levels, words, with_variance):
    owner, position, normal, values3, values1, variance = synthetic(w, h)
    values = values3 if words == 3 else values1
    kw = dict(SIG, levels=levels, dilate=2)
    if with_variance:
        kw.update(variance=variance, sigma_color=2.0)
    got = gpu("cornell").filter_lightmap(values, owner, position, normal, **kw)
    want = F.filter_lightmap(values, owner, position, normal, **kw)
    if with_variance:
        assert M.same(got[0], want[0]) and M.same(got[1], want[1])
        assert got[1].shape == (h, w) and M.same(got[1][owner < 0], variance[owner < 0])
        out = got[0]
    else:
        assert M.same(got, want)
        out = got
    assert out.shape == values.shape
    if w * h > 16:   # (the map says something: the filter moved the valid texels, and no odd value spread)
        plain = gpu("cornell").filter_lightmap(values, owner, position, normal, **dict(kw, dilate=0))
        plain = plain[0] if with_variance else plain
        valid = owner >= 0
        assert M.same(plain[~valid], values[~valid]) and not M.same(plain[valid], values[valid])
        odd = ~np.isfinite(values).reshape(h, w, -1).all(axis=-1)
        assert int(odd.sum()) == 2 and int((~np.isfinite(plain).reshape(h, w, -1).all(axis=-1)).sum()) == 2
        assert M.same(plain[~np.isfinite(values)], values[~np.isfinite(values)])   # (the odd components; the others filter on)


# ---- real bakes
def floor_chart(name):
    """a mesh that IS in the scene, untransformed — cornell's floor, wine_glass's table —: its triangles' rows, and uvs that
    lay its bounding rectangle in the two widest axes over [0.08, 0.92]^2 of the map (tests/test_gpu_lightmap.py's)"""
    scene = small_scenes.small(name)[0]
    rows = next(mesh.triangles for ob, child, chain, mesh in surface_model.meshes_of(scene)
                if ob == {"cornell": 0, "wine_glass": 1}[name] and child < 0 and chain == [None])
    rows = np.ascontiguousarray(rows)
    v = rows[:, :9].reshape(-1, 3, 3)
    ext = v.reshape(-1, 3).max(axis=0) - v.reshape(-1, 3).min(axis=0)
    ax = np.sort(np.argsort(ext)[1:])
    lo = v.reshape(-1, 3).min(axis=0)[ax]
    uvs = 0.08 + 0.84 * (v[:, :, ax] - lo) / ext[ax]
    return rows, np.ascontiguousarray(uvs)


@functools.lru_cache(maxsize=None)
def baked(name, dilate=0):
    """bake_lightmap's IRRADIANCE | AO | OWNER | POSITION | NORMAL of the scene's floor, 24 x 24, 8 samples, 3 bounces — once
    per (scene, dilate), shared, read-only"""
    rows, uvs = floor_chart(name)
    out = gpu(name).bake_lightmap(rows, uvs, 24, 24, samples=8, max_bounces=3, seed=0x4C46, dilate=dilate, channels=ALL,
                                  offset=1e-3 * float(np.abs(rows[:, :9]).max()))
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_no_levels_is_bake_lightmaps_own_dilation(name, k):
    b = baked(name)
    assert 0.3 < (b["owner"] >= 0).mean() < 1.0
    far = dict(sigma_distance=1.0, sigma_plane=1.0, levels=0, dilate=k)
    for channel in ("irradiance", "ao"):
        got = gpu(name).filter_lightmap(b[channel], b["owner"], b["position"], b["normal"], **far)
        assert M.same(got, baked(name, k)[channel])
    if k:
        assert not M.same(baked(name, k)["irradiance"], b["irradiance"])


@pytest.mark.parametrize("channel", ["irradiance", "ao"])
@pytest.mark.parametrize("name", SCENES)
def test_on_a_real_bake_the_call_is_the_models(name, channel):
    b = baked(name)
    extent = lightmap.texel_extent(b["position"], b["owner"])
    assert extent > 0.0
    kw = dict(sigma_distance=3.0 * extent, sigma_plane=extent, sigma_normal=0.1, levels=3, dilate=2)
    got = gpu(name).filter_lightmap(b[channel], b["owner"], b["position"], b["normal"], **kw)
    assert M.same(got, F.filter_lightmap(b[channel], b["owner"], b["position"], b["normal"], **kw))
    owned = b["owner"] >= 0
    assert not M.same(got[owned], b[channel][owned]) and np.isfinite(got).all()


# ---- host and device, the arrays left alone, the scene
@pytest.mark.parametrize("words,with_variance", [(3, True), (1, False)], ids=["3-variance", "1-plain"])
def test_device_tensors_give_the_host_calls_bits(words, with_variance):
    owner, position, normal, values3, values1, variance = synthetic(65, 5)
    values = values3 if words == 3 else values1
    kw = dict(SIG, levels=3, dilate=1)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    if with_variance:
        want = gpu("cornell").filter_lightmap(values, owner, position, normal, variance=variance, **kw)
        got = gpu("cornell").filter_lightmap(t(values), t(owner), t(position), t(normal), variance=t(variance), **kw)
        assert all(isinstance(g, torch.Tensor) and g.device == dev for g in got)
        assert M.same(got[0].cpu().numpy(), want[0]) and M.same(got[1].cpu().numpy(), want[1])
    else:
        want = gpu("cornell").filter_lightmap(values, owner, position, normal, **kw)
        got = gpu("cornell").filter_lightmap(t(values), t(owner), t(position), t(normal), **kw)
        assert isinstance(got, torch.Tensor) and got.device == dev and M.same(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="owner must be a contiguous .* tensor on cuda:0"):   # (no mixing of host and device arrays)
        gpu("cornell").filter_lightmap(t(values), owner, t(position), t(normal), **kw)


def test_inputs_and_what_lies_around_the_outputs_are_untouched():
    """through the C entry point: the inputs keep their bits, `out` and `out_variance` are written inside their [H][W][words]
    and [H][W] and nowhere around them, and a call with a variance and no out_variance gives the same `out`"""
    w, h = 65, 5
    n = w * h
    owner, position, normal, values3, _, variance = (np.array(a) for a in synthetic(w, h))
    ins = {"owner": owner, "position": position, "normal": normal, "values": values3, "variance": variance}
    before = {k: v.copy() for k, v in ins.items()}
    g = gpu("cornell")
    f = _abi.RptLightmapFilter()
    f.struct_size, f.width, f.height, f.words, f.levels, f.dilate = C.sizeof(f), w, h, 3, 2, 1
    f.sigma_normal, f.sigma_plane, f.sigma_distance, f.sigma_color = 0.1, 0.05, 0.4, 2.0
    types = dict(_abi.RptLightmapFilterArrays._fields_)
    pad = 64
    results = []
    for ask_variance in (True, False):
        out, out_v = np.full(3 * n + 2 * pad, 7.0), np.full(n + 2 * pad, 7.0)
        a = _abi.RptLightmapFilterArrays()
        a.struct_size = C.sizeof(a)
        for k, v in ins.items():
            setattr(a, k, v.ctypes.data_as(types[k]))
        a.out = out[pad:].ctypes.data_as(types["out"])
        if ask_variance:
            a.out_variance = out_v[pad:].ctypes.data_as(types["out_variance"])
        _abi.check(g.lib.rptgpu_filter_lightmap(g.handle, C.byref(f), C.byref(a)), g.handle)
        assert (out[:pad] == 7.0).all() and (out[pad + 3 * n:] == 7.0).all()
        assert (out_v[:pad] == 7.0).all() and (out_v[pad + n:] == 7.0).all()
        if not ask_variance:
            assert (out_v == 7.0).all()
        assert all(M.same(ins[k], before[k]) for k in ins)
        results.append((out[pad:pad + 3 * n].reshape(h, w, 3).copy(), out_v[pad:pad + n].reshape(h, w).copy()))
    want = F.filter_lightmap(values3, owner, position, normal, levels=2, dilate=1, variance=variance, sigma_color=2.0, **SIG)
    assert M.same(results[0][0], want[0]) and M.same(results[0][1], want[1]) and M.same(results[1][0], want[0])


def test_the_result_does_not_depend_on_the_handles_scene_and_only_total_ms_moves():
    owner, position, normal, values3, _, variance = synthetic(65, 5)
    kw = dict(SIG, levels=3, dilate=1, variance=variance)
    want = gpu("cornell").filter_lightmap(values3, owner, position, normal, **kw)
    other = gpu("wine_glass").filter_lightmap(values3, owner, position, normal, **kw)
    assert M.same(other[0], want[0]) and M.same(other[1], want[1])
    scene = small_scenes.small("cornell")[0]
    g = GpuScene(scene, 0)
    moved = small_scenes.small("cornell")[0]
    moved.objects[6] = rpt_amd.Object(rpt_amd.cube().scale((165.0, 165.0, 165.0)).rotate_y(0.3).translate((300.0, 82.5, 250.0))) \
        .material(rpt_amd.Material.diffuse(rpt_amd.hex_color(0xAAAAAA)))
    g.set_objects([6], [moved.objects[6]])
    g.reset_stats()
    got = g.filter_lightmap(values3, owner, position, normal, **kw)
    assert M.same(got[0], want[0]) and M.same(got[1], want[1])
    s = g.stats()
    assert s.total_ms > 0.0
    rest = {name: getattr(s, name) for name, _ in _abi.RptStats._fields_ if name != "total_ms"}
    moved_too = [name for name, v in rest.items() if any(x != 0 for x in (v if hasattr(v, "__len__") else [v]))]
    assert moved_too == []
    g.close()
