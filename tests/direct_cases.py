"""What tests/test_direct_host.py and tests/test_gpu_direct.py share: the scenes of rptgpu_bake_direct's tests, one per route
and light kind, the 16 points of each — first hits of the scene's camera rays from the oracle, lifted off their surface —
and the oracle's illuminate as direct_model's light sampler.  Everything here runs on the CPU."""
import functools

import numpy as np

from oracle import oracle_ffi as O
from rpt_amd import Camera, Light, Material, Object, Scene, make_params, plane, scenes, sphere

import small_scenes

N_POINTS = 16
SEED = 0xD12EC7
# name -> (scene, camera): flat with a mesh Light::Object; an in-kernel group under ambient + directional + point; the
# per-tree route under a sphere light; a quad light + a point light; and two sphere lights on either side of a sphere, so that
# a light that faces away from a point stands IN FRONT of one that lights it, on the same stream; the extended-shape build under
# ambient + point + a MonomialSurface light (monomial); trees of trees, which only the per-tree pipeline and the generic walker
# take, under a lamp that is itself a group of groups (nested_groups)
SCENES = ["cornell", "fractal_spheres", "wine_glass", "polygon_room", "two_lamps", "monomial", "nested_groups"]
# the pixels (of a 64 x 36 frame) whose camera rays' first hits are the points, per scene: chosen by a scan with the oracle so
# that lit, shadowed and facing-away points all occur (test_direct_host.test_the_points_show_both_outcomes holds them to it)
PIXELS = {
    "cornell": [(18, 13), (22, 13), (26, 16), (30, 16), (18, 22), (26, 25), (10, 28), (14, 31), (34, 31), (42, 34), (2, 1),
                (30, 4), (50, 10), (58, 19), (6, 25), (46, 22)],
    "fractal_spheres": [(30, 1), (46, 7), (46, 13), (46, 22), (42, 28), (46, 28), (50, 28), (54, 28), (38, 31), (46, 31),
                        (30, 34), (34, 34), (2, 1), (22, 16), (10, 25), (58, 10)],
    "wine_glass": [(34, 4), (38, 4), (34, 10), (30, 13), (34, 13), (34, 16), (34, 19), (38, 19), (14, 22), (18, 25), (22, 25),
                   (22, 28), (26, 28), (2, 19), (50, 22), (30, 31)],
    "polygon_room": [(10, 1), (30, 1), (18, 7), (22, 10), (42, 10), (10, 16), (26, 16), (38, 19), (6, 25), (34, 31), (26, 34),
                     (14, 13), (50, 4), (58, 16), (30, 22), (46, 28)],
    "monomial": [(22, 10), (30, 13), (38, 16), (22, 19), (42, 19), (22, 22), (42, 22), (50, 22), (58, 22), (38, 25), (2, 28),
                 (26, 28), (10, 25), (6, 4), (50, 31), (34, 34)],
    "nested_groups": [(34, 1), (26, 4), (30, 4), (26, 10), (30, 13), (26, 16), (10, 19), (42, 19), (6, 22), (38, 22), (14, 25),
                      (54, 25), (2, 28), (18, 31), (30, 28), (46, 13)],
    "two_lamps": [(22, 7), (26, 10), (22, 13), (26, 16), (18, 16), (34, 7), (38, 10), (34, 13), (38, 16), (42, 13), (46, 16),
                  (30, 10), (30, 25), (30, 31), (10, 22), (58, 28)],
}


def two_lamps():
    sc = Scene()
    sc.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(Material.diffuse((0.6, 0.6, 0.6))))
    sc.add(Object(sphere()).material(Material.diffuse((0.8, 0.3, 0.3))))
    for at, colour in (((-4.0, 0.5, 0.5), (1.0, 0.9, 0.8)), ((4.0, 1.5, 1.0), (0.8, 0.9, 1.0))):
        sc.add(Light.Object(Object(sphere().scale((0.5, 0.5, 0.5)).translate(at)).material(Material.light(colour, 40.0))))
    return sc, Camera.look_at((0.0, 1.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.7)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "two_lamps":
        return two_lamps()
    if name == "fractal_spheres":
        return scenes.fractal_spheres(levels=3)[:2]
    if name == "polygon_room":
        return scenes.polygon_room()[:2]
    return small_scenes.small(name)[:2]


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    return O.OracleScene(scene(name)[0])


@functools.lru_cache(maxsize=None)
def points(name):
    """(positions, normals facing the camera — no unit vectors: the call normalises them —, stream ids that are not the
    indices) — computed once, shared, read-only"""
    sc, cam = scene(name)
    params = make_params(64, 36, 0, 1, seed=SEED)
    rays = [O.camera_ray(cam, params, x, y, 0) for x, y in PIXELS[name]]
    o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    t, nrm, obj = oracle_scene(name).closest_hit(o, d)
    assert len(rays) == N_POINTS and (obj >= 0).all(), (name, obj)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where((np.einsum("ij,ij->i", nrm, d) < 0.0)[:, None], nrm, -nrm)
    pos = o + t[:, None] * d + (1e-6 * t)[:, None] * nrm
    rs = np.random.RandomState(sum(map(ord, name)))
    ids = rs.permutation(1000)[:N_POINTS].astype(np.uint32) + 3
    nrm = nrm * rs.uniform(0.25, 4.0, (N_POINTS, 1))
    for a in (pos, nrm, ids):
        a.setflags(write=False)
    return pos, nrm, ids


def oracle_illuminate(light, pos, seed, stream, sample, draw, **_):
    """direct_model's `illuminate` from the oracle, for every kind of light"""
    return O.illuminate(light, pos, seed=seed, pixel=stream, sample=sample, draw=draw)


def oracle_closest_t(name):
    oc = oracle_scene(name)
    return lambda o, d: oc.closest_hit(o, d)[0]
