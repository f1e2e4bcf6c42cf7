"""The scenes, live updates and query inputs of the update matrix: what tests/test_gpu_update_matrix.py runs on the GPU and
what tests/test_update_cases_host.py holds true about it with the oracle and the host kd builder alone.  A helper, not a test.

A case is a scene a handle is made from (`scene0`, with the handle's `options`) and a list of steps.  A step applies one
live update to the handle (`apply`) and names the scene a FRESH handle is made from to check it (`scene`); the last step of
every case brings the handle back to scene0.  The builders are the existing update tests': the knot scene and its
deformations (test_gpu_mesh_update), the group scene, its children and their motions (test_gpu_group_update), the video
scene and the lit scene (test_gpu_scene_update).

Every case has 600 rays (three 256-thread blocks, the last one partial; test_gpu_occlusion.N_RAYS), 16 points for ambient
occlusion and three views at 37 x 21 (777 pixels: four blocks, the last one partial).  Half of the rays aim at the boxes
the updated object lies in before and after the update, the other half anywhere; no direction is a unit vector.

tests/test_gpu_update_newer.py runs the entry points added later over the same cases, rays, points and views, with one
lightmap chart per case (`chart`: 91 texels), sample counts and stream ids of its own further down."""
import functools
import math

import numpy as np

from rpt_amd import Camera, Light, Material, Object, View, cube, hex_color, make_params, scenes, sphere

import test_gpu_group_update as GU
import test_gpu_mesh_update as MU
import test_gpu_scene_update as SU

N_RAYS = 600
N_POINTS, AO_SAMPLES, AO_SEED = 16, 33, 0x0A0C
W, H, BOUNCES, SPP, BASE = 37, 21, 3, 2, 5
SEEDS = (5, 2 ** 63 + 1, 5)  # test_gpu_views_seeded's: no arithmetic sequence, one above 2^63, one duplicate
KNOT, KIDS = MU.KNOT, GU.KIDS
KNOT_DEPTH = MU.tree_of(KNOT)["max_depth"]


class Step:
    def __init__(self, name, apply, scene, back=False):
        self.name, self.apply, self.scene, self.back = name, apply, scene, back


class Case:
    """start, aim: the boxes the rays' origins and the aimed rays' targets are drawn from (aim: one box or several, taken in
    turn); updated: the objects the steps change; moves: the hit distances change (not so for lights and materials);
    flags_rise: a step raises tree_kids on the handle; device: the _device forms run too; level: every fourth ray is level —
    its y component an exact zero, in the scene as in the frame of a mesh that is turned about y only"""

    def __init__(self, name, scene0, steps, start, aim, updated, options=None, camera=None, moves=True, flags_rise=False,
                 device=False, level=False):
        self.name, self.scene0, self.steps, self.options = name, scene0, steps, dict(options or {})
        self.start, self.aim = start, aim if isinstance(aim, list) else [aim]
        self.updated, self.camera, self.moves, self.flags_rise, self.device = tuple(updated), camera or Camera(), moves, flags_rise, device
        self.level = level
        assert steps[-1].back and not any(s.back for s in steps[:-1])

    def __repr__(self):
        return self.name


# ---- the flat Cornell box: the small cube moved, turned and recoloured (test_gpu_first_hits' update), then out of the box —
# beyond every box the creation's grid was laid over —, then at a placement that is not finite, then back
def _cornell(cube_at=None, turn=0.4, color=0x3366CC):
    scene, cam, _ = scenes.cornell()
    if cube_at is not None:
        scene.objects[6] = Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(turn).translate(cube_at)).material(Material.diffuse(hex_color(color)))
    return scene, cam


def _set_object(i, scene):
    return lambda g: g.set_objects([i], [scene.objects[i]])


def _objects_flat():
    s0, cam = _cornell()
    moved, outside, gone = _cornell((300.0, 120.0, 140.0))[0], _cornell((278.0, 200.0, -250.0))[0], _cornell((300.0, math.inf, 140.0))[0]
    steps = [Step("moved", _set_object(6, moved), moved), Step("outside", _set_object(6, outside), outside),
             Step("not finite", _set_object(6, gone), gone), Step("back", _set_object(6, s0), s0, back=True)]
    return Case("objects_flat", s0, steps, ((30.0, 30.0, -500.0), (520.0, 520.0, 40.0)),
                [((100.0, 0.0, 80.0), (390.0, 210.0, 260.0)), ((190.0, 110.0, -340.0), (370.0, 290.0, -160.0))], [6], camera=cam, device=True)


# ---- the video scene, five primitives: the flat path kernel runs its object filter (boxes on a grid laid over the creation's
# objects).  The cube leaves that grid towards the eye, where it fills a tenth of the frame; a sphere's placement stops being
# finite; back
def _objects_filtered():
    s0, cam = SU.video(0)
    far, _ = SU.video(cube_at=(0.5, 0.3, 6.5))
    gone, _ = SU.video(0)
    gone.objects[2] = Object(sphere().scale((0.5, 0.5, 0.5)).translate((1.5, math.inf, 1.0))).material(Material.specular(hex_color(0x0000FF), 0.1))
    steps = [Step("outside the grid", lambda g: g.update(far), far), Step("not finite", lambda g: g.update(gone), gone),
             Step("back", lambda g: g.update(s0), s0, back=True)]
    return Case("objects_filtered", s0, steps, ((-3.0, -0.5, 5.0), (3.0, 3.0, 9.0)),
                [((0.0, -1.0, 3.6), (0.8, -0.6, 4.4)), ((0.1, 0.1, 6.1), (0.9, 0.5, 6.9)), ((1.0, -1.0, 0.5), (2.0, 0.0, 1.5))], [1, 2], camera=cam)


# ---- lights: the object light and the point light moved and recoloured, the directional light turned onto an axis
def _lit(axis=False, **kw):
    s = SU.lit_scene(**kw)
    s.add(Light.Directional((0.9, 0.8, 0.7) if axis else (0.6, 0.6, 0.9), (0.0, -1.0, 0.0) if axis else (0.3, -1.0, 0.2)))
    return s


def _lights():
    s0 = _lit()
    new = _lit(axis=True, light_at=(1.0, 2.5, 3.0), light_scale=0.3, light_color=(0.3, 0.5, 1.0), point_at=(2.0, 3.0, 4.0), point_color=(5.0, 1.0, 1.0))
    steps = [Step("moved", lambda g: g.set_lights([3, 0, 1], [new.lights[3], new.lights[0], new.lights[1]]), new),
             Step("back", lambda g: g.set_lights([0, 1, 3], [s0.lights[0], s0.lights[1], s0.lights[3]]), s0, back=True)]
    return Case("lights", s0, steps, ((-4.0, -0.5, 3.0), (4.0, 4.0, 8.0)), ((-1.5, -1.0, -1.0), (2.4, 1.0, 1.2)), [], moves=False)


# ---- the knot scene
KNOT_START, KNOT_AIM = ((-4.0, -0.5, 3.0), (4.0, 4.0, 8.0)), ((-2.0, -1.0, -1.4), (0.8, 1.6, 1.4))
ONE_LEAF = np.tile(KNOT[:1], (len(KNOT), 1))


def _set_mesh(tris):
    return lambda g: g.set_mesh(0, tris)


def _mesh_case(name, deformations, **kw):
    kw.setdefault("options", {"deep_depth": 1})
    steps = [Step(n, _set_mesh(t), MU.base_scene(t)) for n, t in deformations]
    steps.append(Step("original", _set_mesh(KNOT), MU.base_scene(KNOT), back=True))
    return Case(name, MU.base_scene(KNOT), steps, KNOT_START, KNOT_AIM, [0], **kw)


# ---- the knot as the scene's ONLY tree, created as two leaves under one split: rpt_tree_generic's columns are two levels
# high until set_mesh brings the knot's own triangles.  The default route hands that kernel the rays with a zero direction
# component, hence the level rays; RPT_FLAG_GENERAL_TRAVERSAL sizes the columns per call and would hide a stale height
TWO_LEAVES = np.concatenate([np.tile(KNOT[:1], (len(KNOT) // 2, 1)), np.tile(KNOT[384:385], (len(KNOT) // 2, 1))])  # (two triangles far apart)


def lone_knot_scene(tris):
    s = MU.base_scene(tris)
    del s.objects[1]  # (the second mesh: its tree would make the columns eleven levels high from the start)
    return s


def _mesh_from_two_leaves():
    steps = [Step("the knot", _set_mesh(KNOT), lone_knot_scene(KNOT)), Step("two leaves", _set_mesh(TWO_LEAVES), lone_knot_scene(TWO_LEAVES), back=True)]
    return Case("mesh_from_two_leaves", lone_knot_scene(TWO_LEAVES), steps, KNOT_START, KNOT_AIM, [0], options={"deep_depth": 1}, level=True)


def _diffuse_knot_scene(glass=False):
    s = MU.base_scene(KNOT)
    if glass:  # materials only: the shapes are the creation's
        s.objects[0] = Object(s.objects[0].shape).material(Material.clear(1.5, 0.0001))
        s.objects[1] = Object(s.objects[1].shape).material(Material.metallic_((0.9, 0.9, 0.9), 0.05))
        s.objects[2] = Object(s.objects[2].shape).material(Material.clear(1.5, 0.0001))
    else:
        s.objects[1] = Object(s.objects[1].shape).material(Material.diffuse((0.3, 0.6, 0.9)))
    return s


def _materials_deeper():
    s0, new = _diffuse_knot_scene(), _diffuse_knot_scene(glass=True)
    put = lambda s: (lambda g: g.set_objects([0, 1, 2], s.objects[:3]))
    return Case("materials_deeper", s0, [Step("glass and mirror", put(new), new), Step("back", put(s0), s0, back=True)],
                KNOT_START, KNOT_AIM, [0, 1, 2], options={"deep_depth": 1}, moves=False)


def _mesh_then_objects():
    tris, moved = MU.sine(KNOT, 4.0), dict(at=(-0.2, 0.4, -0.5), turn=1.1)

    def back(g):
        g.set_mesh(0, KNOT)
        g.update(MU.base_scene(KNOT))

    steps = [Step("set_mesh", _set_mesh(tris), MU.base_scene(tris)),
             Step("update", lambda g: g.update(MU.base_scene(KNOT, **moved)), MU.base_scene(tris, **moved)),  # (placements only)
             Step("back", back, MU.base_scene(KNOT), back=True)]
    return Case("mesh_then_objects", MU.base_scene(KNOT), steps, KNOT_START, KNOT_AIM, [0], options={"deep_depth": 1})


# ---- the group scene, on both routes
def _group_case(route, **kw):
    steps = [Step(n, (lambda kids: lambda g: g.set_group(0, GU.shapes(kids)))(dict(GU.MOTIONS)[n](KIDS)), GU.base_scene(dict(GU.MOTIONS)[n](KIDS)),
                  back=n == "original") for n in ("jitter", "clustered", "coincident", "original")]
    return Case("group_" + route, GU.base_scene(KIDS), steps, ((-4.0, -1.0, 3.0), (4.0, 4.0, 8.0)), ((-1.9, -1.1, -1.2), (0.5, 1.5, 1.2)), [0],
                options=GU.ROUTES[route], **kw)


@functools.lru_cache(maxsize=None)
def cases():
    all_cases = [_objects_flat(), _objects_filtered(), _lights(), _materials_deeper(),
                 _mesh_case("mesh_same_depth", [("sine", MU.sine(KNOT))]),
                 _mesh_case("mesh_deeper", [("clustered", MU.clustered(KNOT)), ("one leaf", ONE_LEAF)], device=True),
                 _mesh_case("mesh_past_fast_stacks", [("clustered", MU.clustered(KNOT))],
                            options={"deep_depth": 1, "fast_max_depth": KNOT_DEPTH}, flags_rise=True),
                 _group_case("in_kernel"), _group_case("per_tree", device=True), _mesh_then_objects(), _mesh_from_two_leaves()]
    return {c.name: c for c in all_cases}


NAMES = ["objects_flat", "objects_filtered", "lights", "materials_deeper", "mesh_same_depth", "mesh_deeper", "mesh_past_fast_stacks",
         "group_in_kernel", "group_per_tree", "mesh_then_objects", "mesh_from_two_leaves"]


# ---- the query inputs, computed once per case and read-only
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _in(rs, boxes, n):
    pts = np.empty((n, 3))
    for k, (lo, hi) in enumerate(boxes):
        rows = np.arange(n) % len(boxes) == k
        pts[rows] = rs.uniform(lo, hi, (int(rows.sum()), 3))
    return pts


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins, directions, max_t): even rays aim at a point of the case's aim boxes, odd ones anywhere; max_t cycles through
    +inf, NaN, 0, -1 and four lengths up to the scene's size (in units of the ray's own parameter)"""
    c = cases()[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 7)
    o = rs.uniform(c.start[0], c.start[1], (N_RAYS, 3))
    target = _in(rs, c.aim, N_RAYS)
    if c.level:
        o[::4, 1] = target[::4, 1]  # rays 0, 4, 8, ...: aimed ones, whose difference in y is then an exact zero
    aimed = target - o
    reach = np.linalg.norm(aimed, axis=1, keepdims=True)
    wild = rs.standard_normal((N_RAYS, 3))
    wild *= reach / np.linalg.norm(wild, axis=1, keepdims=True)
    d = np.where((np.arange(N_RAYS) % 2 == 0)[:, None], aimed, wild) * rs.uniform(0.25, 4.0, (N_RAYS, 1))
    lengths = rs.uniform(0.0, 2.0, N_RAYS)  # of the ray parameter: 1 is the aimed point at the direction's first length
    forms = [np.full(N_RAYS, math.inf), np.full(N_RAYS, math.nan), np.zeros(N_RAYS), np.full(N_RAYS, -1.0), lengths, 0.5 * lengths,
             2.0 * lengths, 4.0 * lengths]
    max_t = np.choose(np.arange(N_RAYS) % len(forms), forms)
    return _frozen(o, d, max_t)


@functools.lru_cache(maxsize=None)
def points(name):
    """(positions in the first aim box, unit normals, stream ids that are not the indices, half that box's diagonal)"""
    lo, hi = cases()[name].aim[0]
    rs = np.random.RandomState(sum(map(ord, name)) + 11)
    pos = rs.uniform(lo, hi, (N_POINTS, 3))
    nrm = rs.standard_normal((N_POINTS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = rs.permutation(1000)[:N_POINTS].astype(np.uint32) + 5
    return _frozen(pos, nrm, ids) + (0.5 * float(np.linalg.norm(np.subtract(hi, lo))),)


def _v(x):
    return np.array([float(c) for c in x])


@functools.lru_cache(maxsize=None)
def views(name):
    """test_gpu_views' three views from the case's camera: the camera under a lens focused half-way into the scene, an
    orthographic view along it, a panorama from a point 0.6 of the way in"""
    c = cases()[name].camera
    eye, direction = _v(c.eye), _v(c.direction)
    L = float(np.linalg.norm(eye))
    lens = Camera(c.eye, c.direction, c.up, c.fov, 0.0, 0.0).focus(tuple(eye + 0.5 * L * direction), 0.02 * L)
    plain = Camera(c.eye, c.direction, c.up, c.fov, 0.0, 0.0)
    return lens, View.orthographic(plain, L * math.tan(c.fov / 2.0)), View.panorama(tuple(eye + 0.6 * L * direction))


# ---- the inputs of tests/test_gpu_update_newer.py: one chart for the lightmap calls, the sample counts, the stream ids
LM_SAMPLES, PROBE_SAMPLES, DIRECT_SAMPLES = 4, 6, 5
LM_W, LM_H = 13, 7          # tests/test_gpu_lightmap.py's small map: 91 texels
NEWER_SEED = 0x4E57
# where the chart lies in the case's first aim box, as a share of that box's height from its floor: chosen with the oracle so
# that the texels' ambient occlusion is neither all 0 nor all 1 and changes with every step that moves geometry
# (tests/test_update_cases_host.py holds each to it and prints what it measures)
CHART_HEIGHT = {"objects_flat": 0.5, "objects_filtered": 0.25, "lights": 0.5, "materials_deeper": 0.25, "mesh_same_depth": 0.25,
                "mesh_deeper": 0.25, "mesh_past_fast_stacks": 0.25, "group_in_kernel": 0.25, "group_per_tree": 0.25,
                "mesh_then_objects": 0.25, "mesh_from_two_leaves": 0.15}


@functools.lru_cache(maxsize=None)
def chart(name):
    """(triangles (2, 3, 3), uvs (2, 3, 2), width, height, offset): one chart of two triangles — a horizontal quad over the
    x-z extent of the case's first aim box at CHART_HEIGHT, its normal up (Triangle::from_vertices' of these vertex orders) —
    laid over texels 1..11 x 1..5 of the 13 x 7 map: 55 texel centres inside, a gutter of one texel on every side; offset:
    1e-3 of the largest coordinate"""
    lo, hi = (np.array(v, dtype=np.float64) for v in cases()[name].aim[0])
    y = lo[1] + CHART_HEIGHT[name] * (hi[1] - lo[1])
    a, b, c, d = (lo[0], y, lo[2]), (hi[0], y, lo[2]), (hi[0], y, hi[2]), (lo[0], y, hi[2])
    tris = np.array([[a, d, c], [a, c, b]], dtype=np.float64)
    u0, u1, v0, v1 = 1.0 / LM_W, (LM_W - 1.0) / LM_W, 1.0 / LM_H, (LM_H - 1.0) / LM_H
    ua, ub, uc, ud = (u0, v0), (u1, v0), (u1, v1), (u0, v1)
    uvs = np.array([[ua, ud, uc], [ua, uc, ub]], dtype=np.float64)
    return _frozen(tris, uvs) + (LM_W, LM_H, 1e-3 * float(np.abs(tris).max()))


@functools.lru_cache(maxsize=None)
def streams(name):
    """(a stream id per ray (600,) uint32 — points(name)'s ids, ray i's moved on by 1000 for every 16 rays before it, so none
    occurs twice and none is an index —, the lightmap calls' stream_base: the first of those ids)"""
    ids = points(name)[2]
    k = np.arange(N_RAYS, dtype=np.uint32)
    return _frozen(ids[k % N_POINTS] + np.uint32(1000) * (k // N_POINTS)) + (int(ids[0]),)


def frame_params(seed=SEEDS[0], base=BASE):
    """view 0 of the views calls as a render_batch (and an oracle) frame"""
    return make_params(W, H, BOUNCES, SPP, seed=seed, sample_index_base=base)


# ---- what the oracle says about a case: the shares the host test holds above its floors, and the GPU test halves
def share(a, b):
    """of the rows of two arrays, the share whose bits differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    rows = a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)
    return float(rows.any(axis=1).mean())


def _colors(scene):
    return np.array([list(ob._material.lower().color) for ob in scene.objects], dtype=np.float64).reshape(-1, 3)


def _oracle_state(oracle, name, scene):
    o, d, _ = rays(name)
    osc = oracle.OracleScene(scene)
    t, _, obj = osc.closest_hit(o, d)
    albedo = np.where((obj >= 0)[:, None], _colors(scene)[np.maximum(obj, 0)], 0.0)
    frame = osc.render(views(name)[0], frame_params(), threads=0)
    return {"t": t, "object": obj, "albedo": albedo, "frame": frame}


@functools.lru_cache(maxsize=None)
def shares(name):
    """per step that is no return to scene0: the oracle's answers on the case's rays and its frame of view 0 before and after
    -> {step name: {hit, miss, reached, t, occluded, albedo, frame}} (shares of the 600 rays, of the 777 pixels)"""
    from oracle import oracle_ffi as oracle
    c = cases()[name]
    before = _oracle_state(oracle, name, c.scene0)
    out = {}
    for step in c.steps:
        if step.back:
            continue
        after = _oracle_state(oracle, name, step.scene)
        hit = after["object"] >= 0
        reached = np.isin(before["object"], c.updated) | np.isin(after["object"], c.updated)
        out[step.name] = {"hit": float(hit.mean()), "miss": float((~hit).mean()), "reached": float(reached.mean()),
                          "t": share(before["t"], after["t"]), "occluded": share(before["object"] >= 0, after["object"] >= 0),
                          "albedo": share(before["albedo"], after["albedo"]),
                          "frame": share(before["frame"], after["frame"])}
    return out


# ---- what the oracle says about the inputs of tests/test_gpu_update_newer.py (tests/test_update_cases_host.py holds the
# floors; every function here runs on the CPU)
def _scenes_of(name):
    """[(None, scene0)] + [(step name, its scene)] for the steps that are no return"""
    c = cases()[name]
    return [(None, c.scene0)] + [(s.name, s.scene) for s in c.steps if not s.back]


@functools.lru_cache(maxsize=None)
def chart_texels(name):
    """the chart by tests/lightmap_model.py: (its four raw channels, the owned texels (H, W) bool, their gather points, their
    unit normals, their stream ids: stream_base + y * width + x)"""
    import lightmap_model
    tris, uvs, w, h, offset = chart(name)
    raw = lightmap_model.raw(tris, None, uvs, w, h, offset=offset)
    owned = raw["owner"] >= 0
    ys, xs = np.nonzero(owned)
    ids = (streams(name)[1] + ys * w + xs).astype(np.uint32)
    return (raw, owned) + _frozen(np.ascontiguousarray(raw["position"][owned]), np.ascontiguousarray(raw["normal"][owned]), ids)


@functools.lru_cache(maxsize=None)
def chart_ao(name):
    """the unoccluded fraction at the chart's owned texels as include/rpt_gpu.h defines bake_ao — RPT_PROBE_IRRADIANCE's
    directions (test_gpu_probes.directions: the oracle's stream and Sphere::sample), the oracle's closest_hit,
    test_gpu_occlusion.fold — -> {None or step name: {"inf": ao, "half": ao}}: LM_SAMPLES directions from sample BASE on, at
    max_distance = inf and at half the aim box's diagonal"""
    from oracle import oracle_ffi as oracle
    import test_gpu_occlusion as occ
    import test_gpu_probes as probes
    _, _, pos, nrm, ids = chart_texels(name)
    half = points(name)[3]
    d, _ = probes.directions(probes.IRR, nrm, ids, NEWER_SEED, LM_SAMPLES, BASE)
    out = {}
    for step, scene in _scenes_of(name):
        t = oracle.OracleScene(scene).closest_hit(np.repeat(pos, LM_SAMPLES, axis=0), d.reshape(-1, 3))[0].reshape(len(pos), LM_SAMPLES)
        out[step] = {"inf": occ.fold(d, t, math.inf)[0], "half": occ.fold(d, t, half)[0]}
    return out


@functools.lru_cache(maxsize=None)
def direct_at_points(name):
    """rptgpu_bake_direct at points(name) by tests/direct_model.py with the oracle's illuminate and closest_hit ->
    {None or step name: (16, 3)}: DIRECT_SAMPLES samples from sample BASE on, on the points' stream ids"""
    from oracle import oracle_ffi as oracle
    import direct_cases
    import direct_model
    pos, nrm, ids, _ = points(name)
    out = {}
    for step, scene in _scenes_of(name):
        osc = oracle.OracleScene(scene)
        out[step] = direct_model.direct(scene.lights, pos, nrm, DIRECT_SAMPLES, NEWER_SEED, lambda o, d: osc.closest_hit(o, d)[0],
                                        sample_index_base=BASE, streams=ids, illuminate=direct_cases.oracle_illuminate)
    return out


# does bake_direct at points(name) change its bits from scene0 to the step's scene?  By direct_at_points (the host test holds
# this table to the model; the GPU test asserts what it says).  materials_deeper: a shadow ray stops at any object, glass
# too.  objects_filtered's sphere and mesh_same_depth's gentle sine stand in none of the 16 points' 5 samples' way to a light
DIRECT_CHANGES = {
    "objects_flat": {"moved": True, "outside": True, "not finite": True},
    "objects_filtered": {"outside the grid": True, "not finite": False},
    "lights": {"moved": True},
    "materials_deeper": {"glass and mirror": False},
    "mesh_same_depth": {"sine": False},
    "mesh_deeper": {"clustered": True, "one leaf": True},
    "mesh_past_fast_stacks": {"clustered": True},
    "group_in_kernel": {"jitter": True, "clustered": True, "coincident": True},
    "group_per_tree": {"jitter": True, "clustered": True, "coincident": True},
    "mesh_then_objects": {"set_mesh": True, "update": True},
    "mesh_from_two_leaves": {"the knot": True},
}
MESH_CASES = [n for n in NAMES if n.startswith("mesh_")]  # object 0, the knot, gets new triangles


@functools.lru_cache(maxsize=None)
def on_updated_mesh(name):
    """per step of a mesh case, the return to the knot too — every one of them is a set_mesh —: the rays(name) whose oracle
    record is a triangle's of the UPDATED mesh (object 0): some row of it gives the oracle's t to the bit with all three
    weights >= 0 (surface_model.tri_records in the mesh's frame, as tests/test_hit_surface_host.py holds it) ->
    {step name: (600,) bool}"""
    from oracle import oracle_ffi as oracle
    import surface_model
    o, d, _ = rays(name)
    out = {}
    for step, scene in [(s.name, s.scene) for s in cases()[name].steps]:
        t, _, obj = oracle.OracleScene(scene).closest_hit(o, d)
        (_, _, chain, mesh), = [m for m in surface_model.meshes_of(scene) if m[0] == 0]
        rows = np.unique(mesh.triangles, axis=0)  # (ONE_LEAF and TWO_LEAVES repeat their rows)
        found = np.zeros(N_RAYS, dtype=bool)
        for i in np.flatnonzero(obj == 0):
            lo, ld = o[i:i + 1], d[i:i + 1]
            for xf in chain:
                if xf is not None:
                    lo, ld = surface_model.local_rays(xf, lo, ld)
            time, uvw, _ = surface_model.tri_records(rows, np.repeat(lo, len(rows), 0), np.repeat(ld, len(rows), 0))
            found[i] = ((surface_model.bits(time) == surface_model.bits(t[i:i + 1])) & (uvw >= 0.0).all(axis=1)).any()
        out[step] = found
    return out
