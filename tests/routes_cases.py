"""The scenes and inputs of the routes matrix: what tests/test_gpu_routes_matrix.py runs on the GPU and what
tests/test_routes_matrix_host.py holds true about it with the oracle and the scene planner alone.  A helper, not a test.

The entry points added since the renders — trace_rays, bake_probes, trace_vertices, first_hits, occluded, bake_ao, render_views
and its kin, the device Buffer — have GPU tests of their own on flat scenes and on one per-tree mesh.  The matrix calls each of
them once more on one small scene per route those tests do not reach (all from tests/small_scenes.py, unchanged):

  monomial         the ext build (MonomialSurface) on a scene without trees; the persistent kernel's ext views unit
  fractal_spheres  groups walked inside the path kernels, the per-depth path re-order really sorting (the handle is made with
                   RPTGPU_PATH_REORDER_MIN=1; a second one with RPTGPU_PATH_REORDER=0 is its reference)
  fractal_teapots  the ext build, rpt_nest_trace: groups whose children are meshes
  nested_groups    rpt_tree_generic as the only walker of an object: groups inside groups
  deep_nest        the same, four levels deep — trace_rays, trace_vertices and render_views only, to bound the time

Sizes: the scene's camera without its lens, frames of 37 x 21 (777 pixels: four 256-thread blocks, the last one partial), 2
samples per call, the scene's own max_bounces, three views (one per projection), 600 loose rays (three blocks, the last of
88), 16 probes and points with 33 samples each."""
import functools

import numpy as np

from rpt_amd import _abi, make_params

import small_scenes
import test_gpu_occlusion as occ
import test_gpu_trace_rays as R
import test_gpu_views as VT

SCENES = ("monomial", "fractal_spheres", "fractal_teapots", "nested_groups", "deep_nest")
RENDER_ONLY = ("deep_nest",)
QUERIED = tuple(n for n in SCENES if n not in RENDER_ONLY)
BUFFERED = ("monomial", "fractal_teapots")  # the device Buffer: one scene without trees and one per-tree scene of the ext build
DEVICE_FORMS = ("monomial", "fractal_spheres")  # one scene of each build
# what the handle of a scene is made under (read at creation: api_scene.cpp, scene_plan.h fold_routes)
CREATE_ENV = {"fractal_spheres": {"RPTGPU_PATH_REORDER_MIN": "1"}}
UNSORTED_ENV = {"RPTGPU_PATH_REORDER": "0"}
# the objects a scene is in the matrix for: at least SHARE of its camera rays must end on them (fractal_spheres: on each)
COUNTED = {"monomial": (1, 2, 3), "fractal_spheres": (0, 1, 2, 3, 4, 5), "fractal_teapots": (0, 1, 2), "nested_groups": (1, 2),
           "deep_nest": (1, 2)}
SHARE = 0.05
# the route the planner must give the counted objects (launch_limits.h RPT_TRACE_*), and the build (rptgpu_scene::ext_shapes)
TRACE_GROUP, TRACE_MESH, TRACE_NEST, TRACE_GENERIC = 0, 1, 2, 3
SHAPE_MESH, SHAPE_GROUP, SHAPE_MONOMIAL = _abi.RPT_SHAPE_MESH, _abi.RPT_SHAPE_GROUP, _abi.RPT_SHAPE_MONOMIAL
KINDS = {"fractal_spheres": TRACE_GROUP, "fractal_teapots": TRACE_NEST, "nested_groups": TRACE_GENERIC, "deep_nest": TRACE_GENERIC}
EXT = {"monomial": True, "fractal_spheres": False, "fractal_teapots": True, "nested_groups": True, "deep_nest": True}
PER_TREE = ("fractal_teapots", "nested_groups", "deep_nest")  # RPT_K_TREE_TRACE > 0; no persistent kernel for their views

W, H, SPP, BASE = 37, 21, 2, 5
N_RAYS, N_POINTS, AO_SAMPLES, PROBE_SAMPLES = occ.N_RAYS, occ.N_POINTS, 33, 33
SEEDS = (5, 2 ** 63 + 1, 5)  # test_gpu_views_seeded's: no arithmetic sequence, one above 2^63, one duplicate
STRIDE_SEED, STRIDE = 11, 7
BATCHES, FSPP, FBASE, LEVELS = 3, 2, 0, 3
ADAPTIVE_REL_TOL = 0.05  # tests/test_gpu_update_matrix.py's
PIECES = {"views": ("RPTGPU_VIEWS_PIECE", "500"), "hits": ("RPTGPU_HITS_PIECE", "256"), "occlusion": ("RPTGPU_OCCLUSION_PIECE", "256"),
          "probes": ("RPTGPU_PROBES_PIECE", "3")}
# where the loose rays start and the points stand: test_gpu_occlusion's boxes where it has one; for the fractals the cube the
# spheres and teapots fill, open towards the wall at z = -6 behind them; for deep_nest nested_groups' box, the floor below it
BOXES = {"monomial": occ.BOXES["monomial"], "nested_groups": occ.BOXES["nested_groups"],
         "fractal_spheres": ((-2.5, -2.5, -2.5), (2.5, 2.5, 3.0)), "fractal_teapots": ((-2.5, -2.5, -2.5), (2.5, 2.5, 3.0)),
         "deep_nest": ((-3.0, -0.9, -3.0), (3.0, 3.0, 2.5))}
assert W * H == 777 and N_RAYS == 600 and N_POINTS == 16


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (scene, the scene's camera without its lens, its max_bounces, its seed)"""
    s, camera, p0 = small_scenes.small(name)
    return s, R.pinhole(camera), p0.max_bounces, p0.seed


def params(name, base, spp=1, seed=None):
    _, _, bounces, seed0 = scene(name)
    return make_params(W, H, bounces, spp, seed=seed0 if seed is None else seed, sample_index_base=base)


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    from oracle import oracle_ffi
    return oracle_ffi.OracleScene(scene(name)[0])


@functools.lru_cache(maxsize=None)
def camera_case(name, s):
    """test_gpu_trace_rays.case at the matrix's size: (params of ONE sample at index s, the oracle's camera rays, the pixels
    as stream ids, the draws the camera took, the oracle's frame) — computed once, shared, read-only"""
    from oracle import oracle_ffi
    _, camera, _, _ = scene(name)
    p = params(name, s)
    o, d, streams, draws = R.camera_rays(oracle_ffi, camera, p, s)
    want = oracle_scene(name).render(camera, p)
    return (p,) + _frozen(o, d, streams, draws, want)


@functools.lru_cache(maxsize=None)
def rays(name):
    """(origins, directions that are NOT unit vectors) as test_gpu_occlusion.rays makes them from the scene's box — for
    monomial with its vertical rays over the corners of the bowl's box, whose Newton step divides by -0: NaN hits"""
    rs = np.random.RandomState(sum(map(ord, name)) + 1)
    lo, hi = BOXES[name]
    o = rs.uniform(lo, hi, (N_RAYS, 3))
    d = rs.standard_normal((N_RAYS, 3)) * rs.uniform(0.25, 4.0, (N_RAYS, 1))
    if name == "monomial":
        for k, (sx, sz) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
            o[9 * k + 2], d[9 * k + 2] = (0.95 * sx, 4.0, 0.95 * sz), (0.0, -1.0, 0.0)
            o[9 * k + 4 + 9 * 8], d[9 * k + 4 + 9 * 8] = (0.93 * sx, 4.0, 0.96 * sz), (0.0, -1.0, 0.0)
    return _frozen(o, d)


def max_t(name, t):
    """test_gpu_occlusion's lengths from closest_hit's t: +inf, NaN, 0, -1, t, the doubles next to t, t / 2 and 2 t in turn
    (a random finite value where the ray misses)"""
    rs = np.random.RandomState(sum(map(ord, name)) + 2)
    lo, hi = BOXES[name]
    finite = rs.uniform(0.0, 2.0 * np.linalg.norm(np.subtract(hi, lo)) / 4.0, N_RAYS)
    base = np.where(np.isinf(t), finite, t)
    inf = float("inf")
    forms = [np.full(N_RAYS, inf), np.full(N_RAYS, np.nan), np.zeros(N_RAYS), np.full(N_RAYS, -1.0), base,
             np.nextafter(base, -inf), np.nextafter(base, inf), 0.5 * base, 2.0 * base]
    return np.choose(np.arange(N_RAYS) % len(forms), forms)


@functools.lru_cache(maxsize=None)
def points(name):
    """test_gpu_occlusion.points for the scene's box: positions, unit normals, stream ids that are not the indices"""
    rs = np.random.RandomState(sum(map(ord, name)))
    lo, hi = BOXES[name]
    pos = rs.uniform(lo, hi, (N_POINTS, 3))
    nrm = rs.standard_normal((N_POINTS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    ids = rs.permutation(1000)[:N_POINTS].astype(np.uint32) + 5
    return _frozen(pos, nrm, ids)


def half_diagonal(name):
    lo, hi = BOXES[name]
    return 0.5 * float(np.linalg.norm(np.subtract(hi, lo)))


@functools.lru_cache(maxsize=None)
def views(name):
    """test_gpu_views' three projections of the scene's camera: under a lens focused half-way into the scene, an orthographic
    view along it, a panorama from a point 0.6 of the way in"""
    return (VT.cameras(name)[2],) + VT.other_views(name)


def view_params(name, seed, base=BASE, spp=SPP):
    """view 0 of a views call as a render_batch (and an oracle) frame"""
    return params(name, base, spp, seed)


@functools.lru_cache(maxsize=None)
def view_frame(name, seed, base=BASE, spp=SPP):
    """the oracle's frame of the perspective view under `seed` -> (H * W, 3), read-only"""
    return _frozen(oracle_scene(name).render(views(name)[0], view_params(name, seed, base, spp)))[0]


def oracle_frames(name):
    """every oracle frame the matrix compares a device result with -> {what: frame}"""
    out = {"camera rays, sample %d" % s: camera_case(name, s)[5] for s in (0, BASE)}
    out["view 0, seed stride"] = view_frame(name, STRIDE_SEED)
    out["view 0, seeds"] = view_frame(name, SEEDS[0])
    if name in BUFFERED:
        for b in range(BATCHES):
            out["buffer batch %d" % b] = view_frame(name, SEEDS[0], BASE + b * SPP)
    return out


@functools.lru_cache(maxsize=None)
def measured(name):
    """what the oracle alone says about the scene's inputs -> {camera: {object: share of the 777 camera rays of sample 0 that
    end on it}, hit, miss: shares of the 600 loose rays, long: the paths of sample 0 with three or more vertices}"""
    _, camera, _, _ = scene(name)
    osc = oracle_scene(name)
    p, o, d, _, _, _ = camera_case(name, 0)
    obj = osc.closest_hit(o, d)[2]
    ro, rd = rays(name)
    loose = osc.closest_hit(ro, rd)[2]
    lengths = np.array([len(osc.trace_sample(camera, p, x, y, 0)[1]) for y in range(H) for x in range(W)])
    return {"camera": {int(k): float((obj == k).mean()) for k in sorted(set(obj.tolist()))}, "hit": float((loose >= 0).mean()),
            "miss": float((loose < 0).mean()), "long": int((lengths >= 3).sum()), "longest": int(lengths.max())}


def said(name):
    m = measured(name)
    counted = sum(m["camera"].get(k, 0.0) for k in COUNTED[name])
    each = ", ".join("%d: %.1f %%" % (k, 100.0 * v) for k, v in m["camera"].items())
    return "%s: %.1f %% of the camera rays end on objects %s (per object %s); %.1f %% of the loose rays hit, %.1f %% miss; " \
           "%d paths of sample 0 have three or more vertices, the longest %d" \
        % (name, 100.0 * counted, list(COUNTED[name]), each, 100.0 * m["hit"], 100.0 * m["miss"], m["long"], m["longest"])
