"""What tests/test_placements_host.py and tests/test_gpu_placements.py share: placements whose linear part is NOT symmetric,
whose normal transform is no multiple of it and whose determinant is negative or zero; the lamp shapes they are put on; a
room lit by one such lamp (one light: the fused persistent kernel takes it) and a yard of placed objects under two lights;
the bake points of each room and the oracle's frames.  Everything here runs on the CPU.

Transformed::sample (shape.rs:139-150) reads five fields of a placement — transform, linear, inverse_transform,
normal_transform, scale — and intersection only two of them.  Under `shear` a transposed `linear` or `transform` changes the
pdf and the point; under `mirror`, `matrix` and `bottom_row` the pdf is NEGATIVE (height = n.n / |L^-T n| > 0, so
base = det / height < 0) and the lamp emits negative light; under `singular` glm::inverse gives zeros, the world normal is
0 / 0 and the pdf is not finite.  Both are the reference's behaviour, and the device's contract is to reproduce it."""
import functools

import numpy as np

from oracle import oracle_ffi as O
from rpt_amd import (Camera, KdTree, Light, Material, Mesh, Object, Scene, cube, hex_color, make_params, monomial_surface, plane,
                     polygon, scenes, sphere)

from test_gpu_scene_consts import WALL_MATERIALS

LINEAR = ((0.9, 0.3, -0.2), (0.1, -1.1, 0.5), (-0.4, 0.2, 0.7))  # rows; det = -0.589, no symmetry


def matrix4(c, at, bottom=(0.0, 0.0, 0.0, 1.0)):
    """the 4x4 of `matrix` / `bottom_row`, column-major as Shape.transform takes it"""
    rows = [[c * v for v in LINEAR[r]] + [float(at[r])] for r in range(3)] + [[float(v) for v in bottom]]
    return [rows[r][col] for col in range(4) for r in range(4)]


def shear(s, c, at):
    return s.scale((1.2 * c, 0.5 * c, 0.8 * c)).rotate_y(0.7).rotate_x(-0.4).scale((1.3, 0.6, 1.0)).translate(at)


def mirror(s, c, at):
    return s.rotate_z(0.3).scale((-c, 0.6 * c, 0.8 * c)).rotate_y(1.1).translate(at)


def matrix(s, c, at):
    return s.transform(matrix4(c, at))


def bottom_row(s, c, at):
    return s.transform(matrix4(c, at, (0.05 / c, -0.02 / c, 0.03 / c, 1.1)))


def singular(s, c, at):
    return s.rotate_y(0.5).scale((1.2 * c, 0.0, 1.2 * c)).translate(at)


PLACEMENTS = {"shear": shear, "mirror": mirror, "matrix": matrix, "bottom_row": bottom_row, "singular": singular}
NEGATIVE = ("mirror", "matrix", "bottom_row")  # det(linear) < 0


def place(shape, placement, c, at):
    return PLACEMENTS[placement](shape, c, at)


# ---- the lamp shapes.  quad: 2 triangles of area 1/2; pentagon: a fan of 3 triangles of areas 0.195, 0.13125 and 0.6825
QUAD = [(-0.5, 0.0, -0.5), (-0.5, 0.0, 0.5), (0.5, 0.0, 0.5), (0.5, 0.0, -0.5)]
PENTAGON = [(0.65, 0.0, -0.5), (0.65, 0.0, -0.2), (-0.4, 0.0, 0.55), (-0.65, 0.0, 0.55), (-0.65, 0.0, -0.5)]
LAMPS = ["sphere", "cube", "quad", "pentagon", "monomial", "group", "nested"]
EXT_LAMPS = ("monomial", "nested")  # the extended-shape build takes these
SIMPLE_LAMPS = ("sphere", "cube", "quad", "pentagon", "monomial")  # their own pdf is positive


def children_of(outer):
    """the two placements of a group's children: of det < 0 both, and neither the group's own.  A leaf's pdf then has the
    sign of -det(outer): two mirrors cancel"""
    return [p for p in NEGATIVE if p != outer][:2]


def group(outer):
    a, b = children_of(outer)
    return KdTree([place(sphere(), a, 0.45, (-0.55, 0.0, 0.1)), place(cube(), b, 0.5, (0.5, 0.1, -0.1))])


def nested(outer):
    """a group of a group and a sphere; the inner group under `shear` (a leaf's sign stays -det(outer)'s)"""
    a, b = children_of(outer)
    inner = KdTree([place(sphere(), b, 0.4, (-0.4, 0.0, 0.0)), place(cube(), a, 0.4, (0.45, 0.1, 0.1))])
    return KdTree([place(inner, "shear", 0.6, (-0.35, 0.0, 0.0)), place(sphere(), a, 0.3, (0.6, 0.0, 0.2))])


def facing_down(verts, outer):
    """the polygon with the winding under which its placed normal L^-T n points down into the room: Light::illuminate
    takes max(0, -disp . n), a flat lamp shines from one side (a negative determinant does not turn the normal over)"""
    p = polygon(verts)
    nt = place(p, outer, 1.0, (0.0, 0.0, 0.0)).normal_transform  # column-major 3 x 3
    n = p.triangles[0][9:12]
    y = (nt[1] * n[0] + nt[4] * n[1]) + nt[7] * n[2]
    return p if not y > 0.0 else polygon(verts[:1] + verts[:0:-1])  # (the same triangles, turned over)


def geometry(name, placement):
    """what of a lamp's geometry depends on its placement — a polygon's winding, a group's children — as a key: set_lights
    moves a lamp between placements of one key (it does not read geometry)"""
    if name in ("quad", "pentagon"):
        verts = QUAD if name == "quad" else PENTAGON
        return facing_down(verts, placement).triangles[0][3:6].tolist() != list(verts[1])
    if name in ("group", "nested"):
        return tuple(children_of(placement))
    return None


def lamp_shape(name, outer="shear"):
    """the untransformed lamp shape; a group's children and a polygon's winding depend on the placement the lamp gets"""
    if name == "sphere":
        return sphere()
    if name == "cube":
        return cube()
    if name == "quad":
        return facing_down(QUAD, outer)
    if name == "pentagon":
        return facing_down(PENTAGON, outer)
    if name == "monomial":
        return monomial_surface(0.3, 4.0)
    if name == "group":
        return group(outer)
    if name == "nested":
        return nested(outer)
    raise KeyError(name)


def leaf_sign(name, placement):
    """the sign every sample's pdf has (0: not finite)"""
    if placement == "singular":
        return 0
    outer = -1 if placement in NEGATIVE else 1
    return outer if name in SIMPLE_LAMPS else -outer


# ---- the room
ROOM_C, ROOM_AT = 50.0, (278.0, 480.0, 280.0)
WALLS = [
    [(0.0, 0.0, 0.0), (0.0, 0.0, 559.2), (556.0, 0.0, 559.2), (556.0, 0.0, 0.0)],
    [(0.0, 0.0, 559.2), (0.0, 548.9, 559.2), (556.0, 548.9, 559.2), (556.0, 0.0, 559.2)],
    [(556.0, 0.0, 0.0), (556.0, 0.0, 559.2), (556.0, 548.9, 559.2), (556.0, 548.9, 0.0)],
    [(0.0, 0.0, 0.0), (0.0, 548.9, 0.0), (0.0, 548.9, 559.2), (0.0, 0.0, 559.2)],
]
CUBE_MATERIALS = (Material.metallic_(hex_color(0xD4AF37), 0.25), Material((0.8, 0.8, 0.9), 1.8, 0.6, 0.0))
CAMERA = scenes.cornell()[1]
W, H, BOUNCES, SPP, SEED = 48, 32, 3, 3, 9
N_POINTS, BAKE_SEED = 16, 0x91ACE


def lamp_light(shape):
    return Light.Object(Object(shape).material(Material.light(hex_color(0xFFFEFA), 100.0)))


def room(lamp, cubes=None):
    """test_gpu_scene_consts' four walls as untransformed polygons, one cube (cubes: the placed cubes that stand in its
    place, one behind the other in the object list), `lamp` (a placed shape) as the only light, scenes.cornell()'s camera"""
    scene = Scene()
    for pts, m in zip(WALLS, WALL_MATERIALS):
        scene.add(Object(polygon(pts)).material(m))
    if cubes is None:
        cubes = [cube().scale((165.0, 330.0, 120.0)).rotate_y(0.6).rotate_x(0.21).translate((368.0, 190.0, 351.0))]
    for i, shape in enumerate(cubes):
        scene.add(Object(shape).material(CUBE_MATERIALS[i % 2]))
    scene.add(lamp_light(lamp))
    return scene, CAMERA


def room_lamp(name, placement):
    return place(lamp_shape(name, placement), placement, ROOM_C, ROOM_AT)


@functools.lru_cache(maxsize=None)
def room_case(name, placement):
    return room(room_lamp(name, placement))


TABLE_LAMP = [(343.0, 548.8, 227.0), (343.0, 548.8, 257.0), (238.0, 548.8, 332.0), (213.0, 548.8, 332.0), (213.0, 548.8, 227.0)]


@functools.lru_cache(maxsize=None)
def table_room():
    """two consecutive cubes under `mirror` and `matrix`, lit by test_gpu_scene_consts' untransformed pentagon: the fused
    kernel builds its cube-normal tables (and the light triangles' pdfs)"""
    return room(polygon(TABLE_LAMP), cubes=[place(cube(), "mirror", 150.0, (368.0, 170.0, 351.0)),
                                            place(cube(), "matrix", 130.0, (185.0, 120.0, 169.0))])


def params(bounces=BOUNCES, flags=0):
    return make_params(W, H, bounces, SPP, seed=SEED, flags=flags)


_frames = {}


def oracle_frame(key, scene, camera, bounces=BOUNCES):
    """the oracle's frame and counters of a scene, rendered once per key"""
    if (key, bounces) not in _frames:
        img, cnt = O.OracleScene(scene).render(camera, params(bounces), threads=0, counters=True)
        img.setflags(write=False)
        _frames[(key, bounces)] = (img, cnt)
    return _frames[(key, bounces)]


def room_frame(name, placement):
    return oracle_frame(("room", name, placement), *room_case(name, placement))


def same(a, b):
    """bit equality, a NaN equal to any NaN (payloads are not part of the contract)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# the pixels (of a 64 x 36 frame) whose camera rays' first hits are a room's bake points, chosen as direct_cases' are: by a
# scan with the oracle, so that lit points and points in the cube's shadow or facing away both occur
ROOM_PIXELS = [(2, 1), (22, 4), (38, 7), (58, 10), (6, 16), (30, 16), (26, 22), (42, 22), (50, 28), (34, 34), (18, 13), (18, 19),
               (18, 25), (18, 31), (10, 28), (14, 31)]


@functools.lru_cache(maxsize=None)
def points(key="room"):
    """(positions, normals facing the camera and no unit vectors, stream ids that are not the indices) of a scene's bake
    points: direct_cases.points' construction — read-only.  The rooms share theirs: the lamp is no object"""
    sc, cam = room_case("sphere", "shear") if key == "room" else yard(key)
    pix = ROOM_PIXELS if key == "room" else YARD_PIXELS[key]
    p = make_params(64, 36, 0, 1, seed=BAKE_SEED)
    rays = [O.camera_ray(cam, p, x, y, 0) for x, y in pix]
    o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    t, nrm, obj = O.OracleScene(sc).closest_hit(o, d)
    assert len(rays) == N_POINTS and (obj >= 0).all(), (key, obj)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where((np.einsum("ij,ij->i", nrm, d) < 0.0)[:, None], nrm, -nrm)
    pos = o + t[:, None] * d + (1e-6 * t)[:, None] * nrm
    rs = np.random.RandomState(sum(map(ord, key)))
    ids = rs.permutation(1000)[:N_POINTS].astype(np.uint32) + 3
    nrm = nrm * rs.uniform(0.25, 4.0, (N_POINTS, 1))
    for a in (pos, nrm, ids):
        a.setflags(write=False)
    return pos, nrm, ids


# ---- the yard: placed objects of every kind as OBJECTS, under two lights (no fused kernel)
YARD_C = 1.5
YARD_VARIANTS = ["plain", "ext"]
YARD_BOX = ((-5.0, -0.9, -2.0), (5.0, 2.2, 2.0))  # where the loose rays start
N_RAYS, RAY_SEED = 600, 0x9A2D
YARD_PIXELS = {
    "plain": [(2, 13), (14, 16), (22, 19), (38, 10), (58, 13), (62, 19), (30, 4), (46, 31), (26, 34), (50, 7), (2, 19), (6, 22),
              (10, 25), (18, 25), (14, 28), (34, 13)],
    "ext": [(2, 16), (18, 16), (34, 1), (42, 10), (58, 16), (62, 19), (10, 4), (46, 31), (26, 34), (6, 28), (26, 13), (30, 16),
            (22, 25), (30, 25), (34, 28), (54, 25)],
}


def yard_shapes(variant):
    """[(shape, placement, where)], one per placement but `singular`"""
    knot = Mesh(scenes.knot_mesh(8, 6, seed=0x9A2D))  # 96 triangles
    if variant == "plain":
        return [(sphere(), "shear", (-3.8, 0.4, 0.0)), (cube(), "mirror", (-1.3, 0.3, 0.3)),
                (knot.scale((2.0, 2.0, 2.0)), "matrix", (1.3, 0.6, -0.2)), (group("bottom_row"), "bottom_row", (3.8, 0.5, 0.2))]
    return [(monomial_surface(0.8, 4.0), "mirror", (-3.8, 0.0, 0.0)), (nested("matrix").scale((1.7, 1.7, 1.7)), "matrix", (-1.3, 0.5, 0.2)),
            (sphere(), "bottom_row", (1.3, 0.4, -0.2)), (cube(), "shear", (3.8, 0.3, 0.3))]


def yard_objects(variant, order=None):
    """the yard's objects: the plane, the placed shapes (order: which placement and place each shape takes — a swap of two
    is a permutation of range(4)), the singular cube"""
    shapes = yard_shapes(variant)
    order = list(order) if order is not None else list(range(len(shapes)))
    mats = [Material.clear(1.5, 0.05), Material.metallic_(hex_color(0xD4AF37), 0.25), Material.specular(hex_color(0x4060C0), 0.3),
            Material.diffuse(hex_color(0xCC6655))]
    objs = [Object(plane((0.0, 1.0, 0.0), -1.0)).material(Material.diffuse(hex_color(0x999999)))]
    for i, (shape, _, _) in enumerate(shapes):
        _, placement, at = shapes[order[i]]
        objs.append(Object(place(shape, placement, YARD_C, at)).material(mats[i]))
    objs.append(Object(place(cube(), "singular", 0.7, (0.0, 1.8, -1.0))).material(Material.diffuse(hex_color(0x55AA55))))
    return objs


@functools.lru_cache(maxsize=None)
def yard(variant="plain", order=None):
    scene = Scene()
    for o in yard_objects(variant, order):
        scene.add(o)
    scene.add(Light.Point((60.0, 70.0, 50.0), (4.0, 9.0, 6.0)))
    scene.add(lamp_light(place(sphere(), "shear", 0.5, (0.5, 4.0, 1.5))))
    return scene, Camera.look_at((0.5, 2.6, 8.5), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0), 0.75)


@functools.lru_cache(maxsize=None)
def yard_rays():
    """600 loose rays of tests/test_gpu_occlusion.py's kind: origins in a box, directions that are no unit vectors"""
    rs = np.random.RandomState(RAY_SEED)
    lo, hi = YARD_BOX
    o = rs.uniform(lo, hi, (N_RAYS, 3))
    d = rs.standard_normal((N_RAYS, 3)) * rs.uniform(0.25, 4.0, (N_RAYS, 1))
    for a in (o, d):
        a.setflags(write=False)
    return o, d


def yard_frame(variant, order=None):
    return oracle_frame(("yard", variant, order), *yard(variant, order))
