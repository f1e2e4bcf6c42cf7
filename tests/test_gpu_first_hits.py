"""rptgpu_first_hits on the GPU: the first hit of rays the caller brings, on host and on device memory.

The call is DEFINED by things the repository already pins (include/rpt_gpu.h): t, normal and object are GpuScene.closest_hit's,
position is origin + t * dir in plain f64 on hits and +0.0 on misses, albedo the hit object's material colour or +0.0.  Every
comparison is on bits (aov_model.bits) but one closed form, whose bound is 1 ulp.  The scenes: flat (cornell), every analytic
shape (coverage), a deep mesh through the per-tree queries (wine_glass), the extended build with NaN records (monomial), trees
of trees through the generic walker (nested_groups); the rays are test_gpu_occlusion's: 600 of them — three 256-thread blocks,
the last one partial —, hits, misses and grazing ones, their directions no unit vectors."""
import functools
import math

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi

import aov_model
import small_scenes
import test_gpu_occlusion as occ

pytestmark = pytest.mark.gpu

SCENES = occ.SCENES
N = occ.N_RAYS
GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
CHANNELS = (("t", _abi.RPT_HIT_T), ("normal", _abi.RPT_HIT_NORMAL), ("object", _abi.RPT_HIT_OBJECT),
            ("position", _abi.RPT_HIT_POSITION), ("albedo", _abi.RPT_HIT_ALBEDO))
gpu = occ.gpu


def same(a, b):
    """the raw bits: -0.0 != +0.0, a NaN equals the same NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(aov_model.bits(a), aov_model.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


def model(g, scene, o, d):
    """the header's record from closest_hit and numpy"""
    t, nrm, obj = g.closest_hit(o, d)
    hit = obj >= 0
    col = aov_model.colors(scene)
    with np.errstate(all="ignore"):
        pos = np.where(hit[:, None], o + t[:, None] * d, 0.0)  # one multiply, then one add
    alb = np.where(hit[:, None], col[np.maximum(obj, 0)], 0.0)
    return {"t": t, "normal": nrm, "object": obj, "position": pos, "albedo": alb}


@functools.lru_cache(maxsize=None)
def case(name):
    """(origins, directions, the expected record) — computed once, shared, read-only"""
    o, d = occ.rays(name)[:2]
    want = model(gpu(name), small_scenes.small(name)[0], o, d)
    for a in want.values():
        a.setflags(write=False)
    return o, d, want


def differing(got, want):
    return [k for k in want if k not in got or not same(got[k], want[k])] + [k for k in got if k not in want]


# ---- 1. the definition, bit for bit
@pytest.mark.parametrize("flags", [0, GENERAL], ids=["default", "general"])
@pytest.mark.parametrize("name", SCENES)
def test_first_hits_are_closest_hit_and_its_arithmetic(name, flags):
    o, d, want = case(name)
    hit = want["object"] >= 0
    assert hit.mean() >= 0.10 and (~hit).mean() >= 0.10, hit.mean()  # both answers, often
    assert np.isposinf(want["t"][~hit]).all() and (aov_model.bits(want["position"][~hit]) == 0).all()
    if name == "monomial":
        nan = np.isnan(want["t"])
        assert nan.any() and hit[nan].all() and np.isnan(want["position"][nan]).any()  # a NaN record is there, and it stays
    g = gpu(name)
    g.reset_stats()
    got = g.first_hits(o, d, flags=flags)
    assert differing(got, want) == []
    st = g.stats()
    assert st.samples == 0 and st.extend_rays == 0 and st.shadow_rays == 0 and st.kernel_launches[_abi.RPT_K_EXTEND] == 1
    assert st.total_ms > 0.0


# ---- 2. a channel that is not named is not written
@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_every_single_channel_and_nothing_else(name):
    o, d, want = case(name)
    g = gpu(name)
    lib, PD = g.lib, _abi.C.POINTER(_abi.C.c_double)
    types = dict(_abi.RptHitArrays._fields_)
    for only, bit in CHANNELS:
        assert differing(g.first_hits(o, d, channels=bit), {only: want[only]}) == []
        # through the ABI with EVERY pointer set: the arrays of the other channels keep their sentinel
        outs = {k: np.full(want[k].shape, 7, dtype=want[k].dtype) for k, _ in CHANNELS}
        q, a = _abi.RptHitQuery(), _abi.RptHitArrays()
        q.struct_size, q.channels = _abi.C.sizeof(q), bit
        a.struct_size = _abi.C.sizeof(a)
        for k, v in outs.items():
            setattr(a, k, v.ctypes.data_as(types[k]))
        _abi.check(lib.rptgpu_first_hits(g.handle, N, o.ctypes.data_as(PD), d.ctypes.data_as(PD), _abi.C.byref(q), _abi.C.byref(a)),
                   g.handle)
        assert same(outs[only], want[only]), only
        assert all((v == 7).all() for k, v in outs.items() if k != only), only
    pair = g.first_hits(o, d, channels=_abi.RPT_HIT_T | _abi.RPT_HIT_ALBEDO)
    assert differing(pair, {"t": want["t"], "albedo": want["albedo"]}) == []


# ---- 3. a ray's result depends on that ray and the scene and on nothing else
@pytest.mark.parametrize("name", SCENES)
def test_pieces_order_and_company_change_nothing(name, monkeypatch):
    o, d, want = case(name)
    g = gpu(name)
    monkeypatch.setenv("RPTGPU_HITS_PIECE", "256")  # three pieces, the last with 88 rays
    g.reset_stats()
    assert differing(g.first_hits(o, d), want) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    perm = np.random.RandomState(3).permutation(N)
    got = g.first_hits(o[perm], d[perm])
    assert differing(got, {k: v[perm] for k, v in want.items()}) == []
    sub = np.sort(perm[:300])  # a subset: 256 + 44
    got = g.first_hits(o[sub], d[sub])
    assert differing(got, {k: v[sub] for k, v in want.items()}) == []
    monkeypatch.delenv("RPTGPU_HITS_PIECE")
    got = g.first_hits(o[sub][::-1], d[sub][::-1])
    assert differing(got, {k: v[sub][::-1] for k, v in want.items()}) == []


def seven(want):
    """seven rays of a case: four that hit and three that miss, in the case's order"""
    hit = want["object"] >= 0
    return np.sort(np.concatenate([np.flatnonzero(hit)[:4], np.flatnonzero(~hit)[:3]]))


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """7 rays in pieces of 3 — the last holds one —, POSITION alone (not the first channel, three components), against the
    same rays in one piece with every channel: a wrong staging offset, component count or row of the channel table shows"""
    o, d, want = case("cornell")
    idx = seven(want)
    o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    g = gpu("cornell")
    whole = g.first_hits(o, d)
    monkeypatch.setenv("RPTGPU_HITS_PIECE", "3")
    g.reset_stats()
    assert differing(g.first_hits(o, d, channels=_abi.RPT_HIT_POSITION), {"position": whole["position"]}) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    assert differing(whole, {k: v[idx] for k, v in want.items()}) == []


# ---- 4. device arrays
@pytest.mark.parametrize("name", ["cornell", "wine_glass", "nested_groups"])
def test_device_arrays_give_the_host_calls_bits(name, monkeypatch):
    o, d, want = case(name)
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    got = g.first_hits(to(o), to(d))
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert got["object"].dtype == torch.int32 and got["t"].dtype == torch.float64
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want) == []
    monkeypatch.setenv("RPTGPU_HITS_PIECE", "256")
    got = g.first_hits(to(o), to(d), channels=_abi.RPT_HIT_T | _abi.RPT_HIT_OBJECT, flags=GENERAL)
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, {"t": want["t"], "object": want["object"]}) == []
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own
        got = g.first_hits(to(o), to(d), channels=_abi.RPT_HIT_POSITION)
        assert same(got["position"].cpu().numpy(), want["position"])
    with pytest.raises(ValueError):
        g.first_hits(to(o), d)  # a host array beside a device tensor


# ---- 5. a live update
def test_after_set_objects_the_results_are_closest_hits():
    """test_gpu_aov's move of the Cornell box's small cube, with a new colour: afterwards the results are closest_hit's on
    the SAME handle, and those of a handle freshly made from the updated scene"""
    scene = small_scenes.small("cornell")[0]
    o, d, before = case("cornell")
    g = GpuScene(scene, 0)
    assert differing(g.first_hits(o, d), before) == []
    moved, _, _ = rpt_amd.scenes.cornell()
    moved.objects[6] = rpt_amd.Object(rpt_amd.cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
        .material(rpt_amd.Material.diffuse(rpt_amd.hex_color(0x3366CC)))
    g.set_objects([6], [moved.objects[6]])
    want = model(g, moved, o, d)
    got = g.first_hits(o, d)
    fresh = GpuScene(moved, 0)
    new = fresh.first_hits(o, d)
    g.close()
    fresh.close()
    assert differing(got, want) == [] and differing(got, new) == []
    assert (want["object"] == 6).any()
    assert not same(want["t"], before["t"]) and not same(want["albedo"], before["albedo"])  # (it did move, and its colour changed)


# ---- 6. nothing to do, and the refusals on a live handle
def test_nothing_to_do_and_refusals_on_a_live_handle():
    g = gpu("cornell")
    o, d, want = case("cornell")
    none = g.first_hits(np.zeros((0, 3)), np.zeros((0, 3)))
    assert none["t"].shape == (0,) and none["normal"].shape == (0, 3) and none["object"].shape == (0,)
    dev = torch.device("cuda", 0)
    none = g.first_hits(torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros((0, 3), dtype=torch.float64, device=dev))
    assert none["position"].shape == (0, 3)
    for kw, word in ((dict(flags=_abi.RPT_FLAG_PERSISTENT), "RPT_FLAG_PERSISTENT"), (dict(channels=0), "channels == 0"),
                     (dict(channels=32), "unknown RPT_HIT_")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            g.first_hits(o, d, **kw)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
    # a named channel without its array, with the others' arrays untouched
    t = np.full(N, 7.0)
    q, a = _abi.RptHitQuery(), _abi.RptHitArrays()
    q.struct_size, q.channels = _abi.C.sizeof(q), _abi.RPT_HIT_T | _abi.RPT_HIT_NORMAL
    a.struct_size = _abi.C.sizeof(a)
    PD = _abi.C.POINTER(_abi.C.c_double)
    a.t = t.ctypes.data_as(PD)
    rc = g.lib.rptgpu_first_hits(g.handle, N, o.ctypes.data_as(PD), d.ctypes.data_as(PD), _abi.C.byref(q), _abi.C.byref(a))
    assert rc == _abi.RPTGPU_E_INVALID_ARGUMENT and b"RPT_HIT_NORMAL is named but normal is NULL" in g.lib.rptgpu_last_error_detail(g.handle)
    assert (t == 7.0).all()
    assert differing(g.first_hits(o, d), want) == []  # the handle is as good as before


# ---- 7. known answers
def test_down_onto_a_lone_plane():
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.plane((0.0, 1.0, 0.0), 0.0)).material(rpt_amd.Material.diffuse((0.25, 0.5, 0.75))))
    g = GpuScene(scene, 0)
    rs = np.random.RandomState(6)
    o = rs.uniform((-5.0, 0.5, -5.0), (5.0, 3.0, 5.0), (N, 3))
    o[:, 1] = np.round(o[:, 1] * 64.0) / 64.0  # heights with few bits: t = height exactly
    down = np.tile(np.array([0.0, -1.0, 0.0]), (N, 1))
    got = g.first_hits(o, down)
    up = g.first_hits(o, -down)
    g.close()
    assert (got["object"] == 0).all() and (got["t"] == o[:, 1]).all()
    assert (got["normal"] == [0.0, 1.0, 0.0]).all() and (got["albedo"] == [0.25, 0.5, 0.75]).all()
    assert (got["position"][:, 0] == o[:, 0]).all() and (got["position"][:, 1] == 0.0).all() and (got["position"][:, 2] == o[:, 2]).all()
    assert (up["object"] == -1).all() and np.isposinf(up["t"]).all()
    assert (aov_model.bits(up["position"]) == 0).all() and (aov_model.bits(up["albedo"]) == 0).all()


def test_from_the_centre_of_a_large_sphere():
    """along an axis — an exact unit vector — the sphere of radius R is met at t = R: within 1 ulp of it, and the object is
    the sphere, not the plane far behind it"""
    R = 10.0
    scene = rpt_amd.Scene()
    scene.add(rpt_amd.Object(rpt_amd.plane((0.0, 1.0, 0.0), -100.0)).material(rpt_amd.Material.diffuse((0.1, 0.1, 0.1))))
    scene.add(rpt_amd.Object(rpt_amd.sphere().scale((R, R, R))).material(rpt_amd.Material.diffuse((0.5, 0.25, 0.125))))
    g = GpuScene(scene, 0)
    d = np.concatenate([np.eye(3), -np.eye(3)])
    o = np.zeros((6, 3))
    got = g.first_hits(o, d)
    g.close()
    assert (got["object"] == 1).all()
    assert np.abs(got["t"] - R).max() <= math.ulp(R)
    assert (got["albedo"] == [0.5, 0.25, 0.125]).all()
    assert same(got["position"], o + got["t"][:, None] * d)
    assert np.abs(np.einsum("ij,ij->i", got["normal"], d)).min() > 0.999  # the normal lies along the ray
