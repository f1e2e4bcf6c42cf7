"""rptgpu_lookup_lightmap on a real MI355X (include/rpt_gpu_lightmap_lookup.h).

1. The call against the numpy restatement of the header's rule (tests/lightmap_lookup_model.py) fed with the call's own
   rptgpu_hit_surface output, bit for bit: cornell (the flat route), wine_glass (the per-tree route) and `mixed` — coverage with
   a plain mesh and a group that holds a mesh added —, 1, 63, 64, 65 and 1 000 rays (aimed rays plus misses), maps of 1 x 1,
   2 x 1, 3 x 5 and 16 x 16 with random finite texels, a NaN and an infinite one, random valid masks, uvs that leave [0, 1] and a
   NaN uv, both filters, two bindings (in `mixed` one of them on a Transformed mesh); a hit inside the group is unbound.
2. What must not change a bit: pieces of 1, 7 and 64 rays, RPT_FLAG_GENERAL_TRAVERSAL, a subset of the channels (the arrays
   that are not named keep their sentinels), torch tensors on the device, a permutation of the rays, and — after set_objects has
   moved the bound mesh — a fresh handle of the moved scene.
3. The round trip, the test of meaning: a POSITION | OWNER bake of cornell's floor looked up again at rays aimed at the floor
   gives the hit points (tests/test_lightmap_lookup_host.py holds the same rays to the cap on left-out hits with the oracle).
4. The refusals that need a scene, n == 0 and no bindings.
5. rptgpu_render_views_lightmapped: three views, one per projection, at 8 x 6 and 13 x 7, 1 and 3 samples, seed_stride 0 and 1,
   both filters, a non-zero unbound_irradiance and exposure_value, against the model's shading and fold fed with
   tests/views_model.py's rays, hit_surface, first_hits' ALBEDO, the scene's own emittance and trace_rays(max_bounces = 0) on the
   misses; RPTGPU_VIEWS_PIECE cutting inside a view, the general route and the _device form give the same frames."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, KdTree, Material, Mesh, Object, _abi, hex_color, lightmap, scenes, sphere

import lightmap_lookup_model as L
import small_scenes
import surface_model as M
import test_gpu_occlusion as occ

pytestmark = pytest.mark.gpu

GENERAL = _abi.RPT_FLAG_GENERAL_TRAVERSAL
NAMES = ("t", "object", "binding", "covered", "uv", "value")
FALLBACK = (-1.5, 0.25, 7.0)
N = 1000
SCENES = ("cornell", "wine_glass", "mixed")
# the two objects a scene's bindings name (mixed: the Transformed knot and the plain quad), and mixed's group
BOUND = {"cornell": (0, 2), "wine_glass": (1, 0), "mixed": (5, 7)}
GROUP = 8
BOXES = dict(occ.BOXES, mixed=occ.BOXES["coverage"])


def make_scene(name):
    if name != "mixed":
        return small_scenes.small(name)[0]
    scene = small_scenes.small("coverage")[0]
    quad = rpt_amd.polygon([(-2.5, -0.5, 2.0), (-2.5, 1.5, 2.0), (-1.0, 1.5, 2.5), (-1.0, -0.5, 2.5)])
    assert M.is_mesh(quad) and len(quad.triangles) == 2
    scene.add(Object(quad).material(Material.diffuse(hex_color(0x80C0FF))))                                    # 7
    kids = [Mesh(scenes.knot_mesh(12, 4)).scale((0.6, 0.6, 0.6)).translate((2.0, 1.6, 1.2)), sphere().translate((2.2, -0.2, 1.8))]
    scene.add(Object(KdTree(kids)).material(Material.diffuse(hex_color(0x55AA55))))                            # 8
    return scene


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(make_scene(name), 0)


def mesh_of(scene, index):
    return M.unwrap(scene.objects[index].shape)[1]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (origins, dirs, hit_surface's result for them) — N - 100 aimed rays and 100 that leave the scene; shared, read-only"""
    scene = make_scene(name)
    o, d = M.aimed_rays(scene, BOXES[name], sum(map(ord, name)) + 25, N - 100)
    rs = np.random.RandomState(len(name))
    lo, hi = np.array(BOXES[name][0]), np.array(BOXES[name][1])
    far = hi + (hi - lo) * rs.uniform(2.0, 3.0, (100, 3))
    o = np.concatenate([o, far])
    d = np.concatenate([d, rs.uniform(0.1, 1.0, (100, 3)) * (hi - lo)])     # away from the scene
    order = rs.permutation(N)
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    surf = gpu(name).hit_surface(o, d)
    for a in (o, d) + tuple(surf.values()):
        a.setflags(write=False)
    return o, d, surf


@functools.lru_cache(maxsize=None)
def bindings(name, maps):
    """two bindings per scene.  small: a 1 x 1 rgb map and a 2 x 1 scalar map; large: a 3 x 5 rgb map and a 16 x 16 scalar map,
    each with a NaN and an infinite texel and a random valid mask.  uvs random in [-0.2, 1.2] with one corner at (-0.5, -0.4)
    and one at (1.5, 1.4), and in the larger meshes one triangle's with a NaN"""
    scene = make_scene(name)
    rs = np.random.RandomState(sum(map(ord, name + maps)))
    out = []
    shapes = {"small": ((1, 1, 3), (1, 2)), "large": ((5, 3, 3), (16, 16))}[maps]
    for ob, shape in zip(BOUND[name], shapes):
        n_tris = len(mesh_of(scene, ob).triangles)
        uvs = rs.uniform(-0.2, 1.2, (n_tris, 3, 2))
        uvs[0, 0], uvs[-1, 1] = (-0.5, -0.4), (1.5, 1.4)   # (a two-triangle mesh leaves the map on both sides, too)
        if n_tris > 4:
            uvs[3, 1, 0] = np.nan
        tex = rs.uniform(-10.0, 10.0, shape)
        valid = None
        if maps == "large":
            flat = tex.reshape(shape[0] * shape[1], -1)
            flat[rs.randint(len(flat)), 0] = np.nan
            flat[rs.randint(len(flat)), -1] = np.inf
            valid = rs.uniform(size=shape[:2]) < 0.7
        out.append(lightmap.Binding(ob, uvs, tex, valid))
    return tuple(out)


def model(name, maps, filter, sl=slice(None)):
    o, d, surf = case(name)
    want = L.lookup(surf["object"][sl], surf["primitive"][sl], surf["barycentric"][sl], bindings(name, maps), filter, FALLBACK)
    want["t"], want["object"] = surf["t"][sl], surf["object"][sl]
    return want


def differing(got, want, names=NAMES):
    return [k for k in names if k not in got or not M.same(np.asarray(got[k]), np.asarray(want[k]))]


def lookup(g, name, maps, filter, sl=slice(None), **kw):
    o, d, _ = case(name)
    return g.lookup_lightmap(np.ascontiguousarray(o[sl]), np.ascontiguousarray(d[sl]), bindings(name, maps), filter=filter,
                             fallback=FALLBACK, **kw)


# ---- 1. against the model
@pytest.mark.parametrize("maps", ["small", "large"])
@pytest.mark.parametrize("filter", [L.NEAREST, L.BILINEAR])
@pytest.mark.parametrize("name", SCENES)
def test_the_call_is_the_models_over_its_own_hit_surface(name, filter, maps):
    g = gpu(name)
    for n in (1, 63, 64, 65, N):
        got, want = lookup(g, name, maps, filter, slice(0, n)), model(name, maps, filter, slice(0, n))
        assert differing(got, want) == [], n
    # the case says something: both bindings hit, covered and uncovered rays, misses, and (large) a NaN value
    full = model(name, maps, filter)
    assert set(np.unique(full["binding"])) == {-1, 0, 1}
    assert full["covered"].any() and (full["object"] < 0).sum() >= 50
    assert M.same(full["value"][full["covered"] == 0], np.tile(FALLBACK, (int((full["covered"] == 0).sum()), 1)))
    if maps == "large":
        assert ((full["binding"] >= 0) & (full["covered"] == 0)).any()          # every tap invalid, or a NaN uv
        assert (full["uv"][full["binding"] >= 0] < 0.0).any() and (full["uv"][full["binding"] >= 0] > 1.0).any()


def test_a_hit_inside_the_group_is_unbound():
    o, d, surf = case("mixed")
    inside = (surf["object"] == GROUP) & (surf["primitive"] >= 0)
    assert inside.sum() >= 10                                                    # the group's mesh is hit
    got = lookup(gpu("mixed"), "mixed", "large", L.BILINEAR)
    assert (got["binding"][inside] == -1).all() and not got["covered"][inside].any()
    assert M.same(got["uv"][inside], np.zeros((int(inside.sum()), 2)))
    assert M.same(got["value"][inside], np.tile(FALLBACK, (int(inside.sum()), 1)))
    assert (got["binding"][surf["object"] == BOUND["mixed"][0]] == 0).all()      # the Transformed mesh is bound


# ---- 2. what must not change a bit
@pytest.mark.parametrize("piece", [1, 7, 64])
@pytest.mark.parametrize("name", ["cornell", "wine_glass"])
def test_pieces_do_not_change_a_bit(name, piece, monkeypatch):
    n = 65 if piece == 1 else 200
    monkeypatch.setenv("RPTGPU_LOOKUP_PIECE", str(piece))
    g = gpu(name)
    g.reset_stats()
    assert differing(lookup(g, name, "large", L.BILINEAR, slice(0, n)), model(name, "large", L.BILINEAR, slice(0, n))) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == -(-n // piece)


@pytest.mark.parametrize("name", SCENES)
def test_the_general_route_does_not_change_a_bit(name):
    assert differing(lookup(gpu(name), name, "large", L.BILINEAR, flags=GENERAL), model(name, "large", L.BILINEAR)) == []


def test_a_subset_of_channels_is_the_full_calls_and_unnamed_arrays_keep_their_sentinels():
    name, n = "wine_glass", 300
    o, d, _ = case(name)
    want = model(name, "large", L.BILINEAR, slice(0, n))
    g = gpu(name)
    recs, keep = g._lower_bindings(rpt_amd._marshal.HOST, list(bindings(name, "large")), "test")
    types = dict(_abi.RptLookupArrays._fields_)
    shapes = {"t": ((n,), np.float64), "object": ((n,), np.int32), "binding": ((n,), np.int32), "covered": ((n,), np.uint8),
              "uv": ((n, 2), np.float64), "value": ((n, 3), np.float64)}
    bit = dict(zip(NAMES, (1, 2, 4, 8, 16, 32)))
    for named in (("value",), ("covered", "uv"), ("t", "binding"), ("object",), ("t", "object", "value")):
        outs = {k: np.full(s, 7, dtype=dt) for k, (s, dt) in shapes.items()}
        a = _abi.RptLookupArrays()
        a.struct_size = C.sizeof(a)
        for k, arr in outs.items():
            setattr(a, k, arr.ctypes.data_as(types[k]))
        q = _abi.RptLookupQuery()
        q.struct_size, q.channels, q.filter = C.sizeof(q), sum(bit[k] for k in named), _abi.RPT_LOOKUP_BILINEAR
        q.fallback = _abi.V3(*FALLBACK)
        PD = C.POINTER(C.c_double)
        oo, dd = np.ascontiguousarray(o[:n]), np.ascontiguousarray(d[:n])
        _abi.check(g.lib.rptgpu_lookup_lightmap(g.handle, n, oo.ctypes.data_as(PD), dd.ctypes.data_as(PD), 2, recs, C.byref(q),
                                                C.byref(a)), g.handle)
        assert differing(outs, want, named) == []
        assert all((outs[k] == 7).all() for k in NAMES if k not in named)
    del keep


def test_one_channel_of_a_host_caller_in_pieces_of_three(monkeypatch):
    """7 rays in pieces of 3 — the last holds one —, VALUE alone (not the first channel, three components), against the same
    rays in one piece with every channel: a wrong staging offset, component count or row of the channel table shows"""
    name = "cornell"
    want = model(name, "large", L.BILINEAR)
    covered = want["covered"] != 0
    idx = np.sort(np.concatenate([np.flatnonzero(covered)[:4], np.flatnonzero(~covered)[:3]]))
    assert len(idx) == 7
    g = gpu(name)
    whole = lookup(g, name, "large", L.BILINEAR, idx)
    monkeypatch.setenv("RPTGPU_LOOKUP_PIECE", "3")
    g.reset_stats()
    got = lookup(g, name, "large", L.BILINEAR, idx, channels=_abi.RPT_LOOKUP_VALUE)
    assert sorted(got) == ["value"] and differing(got, whole, ("value",)) == []
    assert g.stats().kernel_launches[_abi.RPT_K_EXTEND] == 3
    assert differing(whole, {k: v[idx] for k, v in want.items()}) == []


@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_device_tensors_give_the_host_calls_bits(name, monkeypatch):
    o, d, _ = case(name)
    g = gpu(name)
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)  # (a writable, contiguous copy of the shared arrays)
    on_dev = [lightmap.Binding(b.object, to(b.uvs), to(b.map), None if b.valid is None else to(b.valid)) for b in bindings(name, "large")]
    want = model(name, "large", L.BILINEAR)
    got = g.lookup_lightmap(to(o), to(d), on_dev, filter="bilinear", fallback=FALLBACK)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert got["covered"].dtype == torch.uint8 and got["binding"].dtype == torch.int32 and got["value"].dtype == torch.float64
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want) == []
    monkeypatch.setenv("RPTGPU_LOOKUP_PIECE", "256")
    with torch.cuda.stream(torch.cuda.Stream(dev)):  # on a stream of the caller's own; T and OBJECT in the handle's own pair
        got = g.lookup_lightmap(to(o), to(d), on_dev, filter="nearest", fallback=FALLBACK,
                                channels=_abi.RPT_LOOKUP_VALUE | _abi.RPT_LOOKUP_COVERED, flags=GENERAL)
        assert differing({k: v.cpu().numpy() for k, v in got.items()}, model(name, "large", L.NEAREST), ("covered", "value")) == []
    with pytest.raises(ValueError):  # tensors and numpy arrays do not mix
        g.lookup_lightmap(to(o), to(d), list(bindings(name, "large")))


def test_permuting_the_rays_permutes_the_results():
    name = "wine_glass"
    o, d, _ = case(name)
    perm = np.random.RandomState(3).permutation(N)
    got = gpu(name).lookup_lightmap(np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), bindings(name, "large"),
                                    filter="bilinear", fallback=FALLBACK)
    want = model(name, "large", L.BILINEAR)
    assert differing(got, {k: v[perm] for k, v in want.items()}) == []


def test_after_set_objects_has_moved_the_bound_mesh_the_result_is_a_fresh_handles():
    name = "mixed"
    o, d, _ = case(name)
    g = GpuScene(make_scene(name), 0)
    b = bindings(name, "large")
    before = g.lookup_lightmap(o, d, b, fallback=FALLBACK)
    assert differing(before, model(name, "large", L.BILINEAR)) == []
    moved = make_scene(name)
    knot = BOUND[name][0]
    moved.objects[knot] = Object(Mesh(scenes.knot_mesh(24, 6)).scale((1.4, 1.6, 1.4)).rotate_y(0.4).translate((0.2, 1.1, 0.4))) \
        .material(Material.diffuse(hex_color(0xB7CA79)))
    g.set_objects([knot], [moved.objects[knot]])
    got = g.lookup_lightmap(o, d, b, fallback=FALLBACK)
    assert differing(got, GpuScene(moved, 0).lookup_lightmap(o, d, b, fallback=FALLBACK)) == []
    assert differing(got, before, ["uv"]) == ["uv"]   # (the update is seen)


# ---- 3. the round trip
def test_a_baked_position_map_looked_up_at_the_floor_gives_the_hit_points():
    """Bilinear interpolation of an affine field is exact up to about ten roundings of 1.1e-16 amplified by at most the map's
    width: below 1e-13 of the extent.  A half-texel or swapped-weight mistake moves the value by 1e-2 of the extent at least.
    1e-9 leaves four orders on each side."""
    ob, rows, uvs, o, d, extent = L.round_trip_case()
    g = gpu("cornell")
    size = L.ROUND_TRIP_SIZE
    baked = g.bake_lightmap(rows, uvs, size, size, seed=1, offset=0.0, channels=_abi.RPT_LIGHTMAP_POSITION | _abi.RPT_LIGHTMAP_OWNER)
    b = lightmap.Binding(ob, uvs, baked["position"], baked["owner"] >= 0)
    got = g.lookup_lightmap(o, d, [b], filter="bilinear")
    hits = g.first_hits(o, d, channels=_abi.RPT_HIT_POSITION | _abi.RPT_HIT_OBJECT)
    on = np.flatnonzero(hits["object"] == ob)
    assert len(on) >= 100 and (got["binding"][on] == 0).all() and (got["binding"][hits["object"] != ob] == -1).all()
    full = L.valid_taps(b, got["uv"][on]) == 4
    error = np.abs(got["value"][on][full] - hits["position"][on][full]).max()
    print("round trip: %d floor hits, %d with four valid taps, max |value - position| = %.3e (bound %.3e)"
          % (len(on), int(full.sum()), error, 1e-9 * extent))
    assert full.mean() >= 0.9
    assert (got["covered"][on][full] == 1).all()
    assert error <= 1e-9 * extent


# ---- 4. refusals against the scene; empty calls
def test_refusals_that_need_the_scene_and_empty_calls():
    name = "mixed"
    o, d, _ = case(name)
    g = gpu(name)
    o4, d4 = np.ascontiguousarray(o[:4]), np.ascontiguousarray(d[:4])
    tex, B = np.zeros((2, 2)), lightmap.Binding
    knot, quad = BOUND[name]
    for bad, word in (([B(99, np.zeros((2, 3, 2)), tex)], "object 99 is out of range (the scene has 9)"),
                      ([B(1, np.zeros((2, 3, 2)), tex)], "object 1 is not a top-level mesh"),
                      ([B(GROUP, np.zeros((2, 3, 2)), tex)], "object 8 is not a top-level mesh"),
                      ([B(quad, np.zeros((2, 3, 2)), tex), B(knot, np.zeros((5, 3, 2)), tex)], "binding 1: object 5: n_tris = 5 differs"),
                      ([B(quad, np.zeros((0, 3, 2)), tex)], "binding 0: uvs is NULL")):
        with pytest.raises(rpt_amd.RptGpuError) as e:
            g.lookup_lightmap(o4, d4, bad)
        assert e.value.code == _abi.RPTGPU_E_INVALID_ARGUMENT and word in str(e.value)
    with pytest.raises(rpt_amd.RptGpuError, match="RPT_FLAG_PERSISTENT"):
        g.lookup_lightmap(o4, d4, [], flags=_abi.RPT_FLAG_PERSISTENT)
    none = g.lookup_lightmap(np.zeros((0, 3)), np.zeros((0, 3)), bindings(name, "small"))
    assert none["value"].shape == (0, 3) and none["uv"].shape == (0, 2) and none["covered"].dtype == np.uint8
    unbound = g.lookup_lightmap(o, d, [], fallback=FALLBACK)   # no bindings: every ray is unbound
    _, _, surf = case(name)
    assert (unbound["binding"] == -1).all() and not unbound["covered"].any() and M.same(unbound["value"], np.tile(FALLBACK, (N, 1)))
    assert M.same(unbound["t"], surf["t"]) and M.same(unbound["object"], surf["object"])
    # the handle still renders what it rendered
    t, _, obj = g.closest_hit(o, d)
    assert M.same(t, surf["t"]) and M.same(obj, surf["object"])


# ---- 5. the views form: rptgpu_render_views_lightmapped
import math  # noqa: E402

from rpt_amd import Camera, View  # noqa: E402

import views_model  # noqa: E402

VIEW_SEED, VIEW_BASE = 0x4C4B, 4
UNBOUND = (0.5, 0.25, 2.0)


@functools.lru_cache(maxsize=None)
def the_views(name):
    """one view per projection: the scene's camera without its lens, an orthographic view along it, a panorama from a point
    0.6 of the way into the scene"""
    c = small_scenes.small("coverage" if name == "mixed" else name)[1]
    eye, direction = np.array([float(x) for x in c.eye]), np.array([float(x) for x in c.direction])
    L = float(np.linalg.norm(eye))
    plain = Camera(c.eye, c.direction, c.up, c.fov, 0.0, 0.0)
    return plain, View.orthographic(plain, L * math.tan(plain.fov / 2.0)), View.panorama(tuple(eye + 0.6 * L * direction))


def view_rays(oracle, g, view, seed, w, h, s):
    if isinstance(view, Camera):
        return views_model.perspective_rays(oracle, view, seed, w, h, s)
    if view.projection == _abi.RPT_VIEW_ORTHOGRAPHIC:
        return views_model.orthographic_rays(oracle, view.camera, view.ortho_scale, seed, w, h, s)
    return views_model.panorama_rays(oracle, view.camera.eye, seed, w, h, s, views_model.device_sincos(g))[:2]


def views_model_frames(oracle, name, maps, filter, w, h, iterations, stride, ev):
    """the model fed with views_model's rays, hit_surface, first_hits' ALBEDO, the scene's own emittance and
    trace_rays(max_bounces = 0) on the misses -> (3, h, w, 3)"""
    g, scene = gpu(name), make_scene(name)
    emit = np.array([ob._material.emittance for ob in scene.objects])
    frames = []
    for v, view in enumerate(the_views(name)):
        seed = VIEW_SEED + v * stride
        samples = []
        for s in range(VIEW_BASE, VIEW_BASE + iterations):
            o, d = (np.ascontiguousarray(a) for a in view_rays(oracle, g, view, seed, w, h, s))
            surf = g.hit_surface(o, d)
            look = L.lookup(surf["object"], surf["primitive"], surf["barycentric"], bindings(name, maps), filter)
            albedo = g.first_hits(o, d, channels=_abi.RPT_HIT_ALBEDO)["albedo"]
            hit = surf["object"] >= 0
            env = np.zeros((w * h, 3))
            if (~hit).any():
                env[~hit] = g.trace_rays(np.ascontiguousarray(o[~hit]), np.ascontiguousarray(d[~hit]), 0, samples=1, seed=1)
            samples.append(L.shade(hit, env, albedo, emit[np.maximum(surf["object"], 0)], look["covered"], look["value"], UNBOUND))
        frames.append(L.fold(samples, ev))
    return np.stack(frames).reshape(3, h, w, 3)


def render_lightmapped(g, name, maps, filter, w, h, iterations, stride, ev, b=None, **kw):
    return g.render_views_lightmapped(the_views(name), w, h, bindings(name, maps) if b is None else b, samples=iterations,
                                      seed=VIEW_SEED, seed_stride=stride, sample_index_base=VIEW_BASE, exposure_value=ev,
                                      filter=filter, unbound_irradiance=UNBOUND, **kw)


@pytest.mark.parametrize("filter", [L.NEAREST, L.BILINEAR])
@pytest.mark.parametrize("size,iterations,stride", [((8, 6), 1, 0), ((13, 7), 3, 1)], ids=["8x6-1spp-stride0", "13x7-3spp-stride1"])
@pytest.mark.parametrize("name", SCENES)
def test_the_views_form_is_the_model_over_the_header_rays(name, size, iterations, stride, filter, oracle, monkeypatch):
    (w, h), ev = size, 1.5
    want = views_model_frames(oracle, name, "large", filter, w, h, iterations, stride, ev)
    g = gpu(name)
    got = render_lightmapped(g, name, "large", filter, w, h, iterations, stride, ev)
    assert got.shape == (3, h, w, 3) and got.dtype == np.float64
    for v in range(3):
        assert same_frames(got[v], want[v]), "view %d: %d pixels differ" % (v, (bits(got[v]) != bits(want[v])).any(axis=-1).sum())
    assert not same_frames(got[0], got[1]) and not (got == got[0, 0, 0]).all()
    monkeypatch.setenv("RPTGPU_VIEWS_PIECE", "31")     # cuts inside a view
    assert same_frames(render_lightmapped(g, name, "large", filter, w, h, iterations, stride, ev), want)
    monkeypatch.delenv("RPTGPU_VIEWS_PIECE")
    assert same_frames(render_lightmapped(g, name, "large", filter, w, h, iterations, stride, ev, flags=GENERAL), want)
    # the device form: the bindings' arrays as tensors, a new tensor back
    dev = torch.device("cuda", 0)
    to = lambda a: torch.from_numpy(np.array(a)).to(dev)
    on_dev = [lightmap.Binding(b.object, to(b.uvs), to(b.map), None if b.valid is None else to(b.valid)) for b in bindings(name, "large")]
    out = render_lightmapped(g, name, "large", filter, w, h, iterations, stride, ev, b=on_dev)
    assert isinstance(out, torch.Tensor) and out.device == dev and same_frames(out.cpu().numpy(), want)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_frames(a, b):
    """the raw bits — but a NaN equals any NaN: the `large` maps hold a NaN and an infinite texel, and which payload a sum of
    NaNs keeps is no part of the contract"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def test_the_views_case_says_something(oracle):
    """bound and covered hits, hits that take unbound_irradiance, misses, an emitter — and a product taken after the sample
    sum (albedo times the mean irradiance) is NOT the frame: the jitter moves samples of a pixel across objects"""
    name, (w, h) = "cornell", (13, 7)
    g = gpu(name)
    got = render_lightmapped(g, name, "large", L.BILINEAR, w, h, 3, 1, 0.0)
    none = render_lightmapped(g, name, "large", L.BILINEAR, w, h, 3, 1, 0.0, b=[])
    assert not same_frames(got, none)                                   # the maps are seen
    other = g.render_views_lightmapped(the_views(name), w, h, bindings(name, "large"), samples=3, seed=VIEW_SEED, seed_stride=1,
                                       sample_index_base=VIEW_BASE, unbound_irradiance=(0.0, 0.0, 0.0))
    assert not same_frames(got, other)                                  # unbound_irradiance is read
    with pytest.raises(rpt_amd.RptGpuError, match="RPT_FLAG_VIEWS_PERSISTENT"):
        render_lightmapped(g, name, "large", L.BILINEAR, w, h, 1, 0, 0.0, flags=_abi.RPT_FLAG_VIEWS_PERSISTENT)
    with pytest.raises(rpt_amd.RptGpuError, match="is not a top-level mesh"):
        render_lightmapped(g, name, "large", L.BILINEAR, w, h, 1, 0, 0.0, b=[lightmap.Binding(5, np.zeros((2, 3, 2)), np.zeros((2, 2)))])
