"""The shading matrix: materials at the edges of their parameters, a scene that shows every one of them, and a path
rebuilt from the oracle's per-function entry points (oracle/oracle_ffi.py closest_hit, illuminate, sample_f, bsdf).
Importable without a GPU; tests/test_shading_matrix_host.py checks it against the oracle's own path records and counts
what it covers, tests/test_gpu_vertices_oracle.py holds the device's path vertices to it.

MATERIALS is the grid roughness {1e-3, 0.05, 1, 2} x index {1, 1.0000001, 0.7, 2.4} x {opaque metallic 0, opaque metallic
1, transparent} and three singles: 51 materials, every one inside what scene_create accepts (sample_f's lobe probability
in [0, 1]).  The edges by name:
  roughness 1e-3   m2 = 1e-6: the Beckmann exponent -tan^2 / m2 underflows off the lobe's centre, pdf = 0, 1/pdf = inf
  index 1.0        f0 = 0; transparent: the refraction half vector wi * 1 + wo is the zero vector, normalize gives NaN
  index 1.0000001  the same half vector is tiny but not zero; total internal reflection only within 4.5e-4 of grazing
  index 0.7        eta_t < 1 from OUTSIDE: sample_f's refraction fails (None) on the way in, not on the way out
  index 2.4        total internal reflection from inside over most of the hemisphere
  roughness 2      above the range the constructors document
  black diffuse    bsdf's diffuse term and the ambient product are exactly zero
  white metal      lobe probability exactly 1.0: gen_bool takes no draw
  emissive colour  A_d carries emittance * colour besides the lights

What the scenes cover, counted from the oracle alone (tests/test_shading_matrix_host.py asserts the bounds and prints the
counts).  The matrix at FRAME: 48x40, 2 samples from sample 0, 6 bounces, 3 840 paths a frame.
                                    inner vertices (d < len - 1)   under an all-zero suffix   bound
  cornell 37x21, samples 5 to 7     8 580                          3 139  36.6 %              30 %
  dark scene, outside camera        7 594                          6 530  86.0 %              50 %
  lit scene, outside camera         7 594                          3 479  45.8 %              40 %
  dark scene, inside camera         3 125                          2 845  91.0 %              none
  lit scene, inside camera          3 125                            378  12.1 %              none
  The two matrix bounds are read as bounds on the OUTSIDE camera's frame, deliberately: they were planned on one frame
  of 3 840 paths, and inside the glass cube every hit of the lit scene is lit by the ambient light, so that frame cannot
  reach 40 % and both cameras together (36 %) say less about the scene than about how many paths start inside.
  inner vertices with a non-finite f, 1/pdf or |cos|: 216 a frame from outside, 34 from inside, 500 in all (bound 10)
  least inner vertices of one material over the four frames: 46 (bound 10)
  every transparent material reflects, transmits and fails to refract (None) at least once over the four frames and the
  probe rays — the frames alone give no None at index 1.0000001 (the window is 4.5e-4 wide) and none at index 1.0, where
  there is none to find; probe_rays searches stream ids for the former and says why not for the latter
"""
import ctypes as C
import functools
import math

import numpy as np

from rpt_amd import Camera, Light, Material, Mesh, Object, Scene, _abi, cube, hex_color, make_params, plane, polygon, sphere

ROUGHNESS = (1e-3, 0.05, 1.0, 2.0)
INDEX = (1.0, 1.0000001, 0.7, 2.4)
KINDS = ("opaque", "metal", "transparent")
GRID_COLORS = ((0.9, 0.5, 0.2), (0.3, 0.8, 0.4), (0.2, 0.4, 0.9), (0.8, 0.8, 0.7))  # by roughness: no channel 0 or 1


def _materials():
    out = []
    for ri, r in enumerate(ROUGHNESS):
        for ix in INDEX:
            for kind in KINDS:
                m = Material(GRID_COLORS[ri], index=ix, roughness=r, metallic=1.0 if kind == "metal" else 0.0,
                             transparent=kind == "transparent")
                out.append(("%s r=%g n=%.8g" % (kind, r, ix), m))
    out.append(("black diffuse", Material.diffuse((0.0, 0.0, 0.0))))
    out.append(("white metal", Material.metallic_((1.0, 1.0, 1.0), 0.3)))
    out.append(("emissive colour", Material((0.9, 0.3, 0.6), index=1.5, roughness=0.4, emittance=2.5)))
    return out


MATERIALS = _materials()
assert len(MATERIALS) == 51
TRANSPARENT = [i for i, (_, m) in enumerate(MATERIALS) if m.transparent]
INSIDE = 23  # "transparent r=0.05 n=2.4", a cube: the inside camera's
FIRST_OBJECT = 2  # objects 0 and 1 are the floor and the back wall; object FIRST_OBJECT + i carries MATERIALS[i]
COLUMNS = 9
PARTS = 3  # scene(lit, (k, PARTS)): the opaque, the metallic and the transparent third of the grid, 17 materials each
FRAME = dict(width=48, height=40, samples=2, bounces=6, seed=0x5AD3)


def lobe_probability(m):
    """sample_f's f (material.rs:233-235) in the oracle's operation order: what scene_create bounds to [0, 1]"""
    f0 = ((m.index - 1.0) / (m.index + 1.0)) ** 2
    mean = ((m.color[0] + m.color[1]) + m.color[2]) / 3.0
    f = (1.0 - m.metallic) * f0 + m.metallic * mean
    return f * (1.0 - 0.2) + 1.0 * 0.2


def place(i):
    """centre of the object that carries MATERIALS[i]: rows of COLUMNS, receding from the camera"""
    r, c = divmod(i, COLUMNS)
    return ((c - (COLUMNS - 1) / 2.0) * 1.05 + 0.13 * (r % 2), -0.5, 1.6 - 1.15 * r)


def is_cube(i):
    return i % 2 == 1 or i == len(MATERIALS) - 1  # (the last two are cubes: one two-cube block for the wave's normal tables)


# scene(lit, meshed=True): the spheres of these materials are meshes of MESH_TRIANGLES triangles, each with a kd-tree of
# its own — a transparent r=1e-3 n=0.7, a transparent r=1 n=1.0, a metal r=1e-3 n=1.0000001, an opaque r=2 n=0.7, the black diffuse
MESHED = (4, 8, 26, 42, 48)
MESH_NU, MESH_NV = 12, 8
MESH_TRIANGLES = 2 * MESH_NU * (MESH_NV - 1)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    """the unit sphere as MESH_NU x MESH_NV quads' triangles and a fan at either pole, smooth normals: rows of 18 doubles
    (three vertices, three normals), as Mesh takes them"""
    def point(iu, iv):
        th, ph = math.pi * iv / MESH_NV, 2.0 * math.pi * (iu % MESH_NU) / MESH_NU
        return (math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph))

    rows = []
    for iu in range(MESH_NU):
        for iv in range(MESH_NV):
            a, b, c, d = point(iu, iv), point(iu + 1, iv), point(iu + 1, iv + 1), point(iu, iv + 1)
            if iv > 0:
                rows.append(a + d + b + a + d + b)
            if iv < MESH_NV - 1:
                rows.append(b + d + c + b + d + c)
    rows = np.array(rows, dtype=np.float64)
    assert rows.shape == (MESH_TRIANGLES, 18)
    return rows


def shape(i, meshed=False):
    if is_cube(i):  # rotated about two axes, scaled unevenly
        return cube().scale((0.7, 0.8, 0.75)).rotate_y(0.3 + 0.37 * i).rotate_x(0.2).translate(place(i))
    if meshed and i in MESHED:
        return Mesh(sphere_mesh()).scale((0.42, 0.42, 0.42)).rotate_y(0.1 * i).translate(place(i))
    return sphere().scale((0.42, 0.42, 0.42)).translate(place(i))


@functools.lru_cache(maxsize=None)
def scene(lit, part=None, meshed=False):
    """One small object per material above a diffuse floor, a diffuse wall of two triangles behind them, a black
    environment.  lit: an ambient, a point and a directional light and a sphere Light.Object; else the object light alone
    (the dark variant).  part = (k, n): only the materials k, k + n, k + 2n, ... (their objects where they stand in the
    whole scene) — few enough objects for the persistent kernel's per-wave tables of scene constants, which the whole
    scene's 53 objects do not fit.  meshed: the spheres of MESHED are triangle meshes with real kd-trees, for the
    per-tree route (no other object of the scene has a tree below its root).
    The wall is not scenery: the persistent kernel traces a hit's shadow and bounce ray in one query — the form that can
    have the tables of scene constants — only in a flat scene with a plane table, which takes an untransformed mesh with
    its triangles in LDS (scene_plan.h plan_flat).  Without the wall the dark scene falls back to the unfused kernel and
    tests/test_gpu_vertices_oracle.py's launch-line assertions fail.
    -> (scene, the material index of every object or -1)"""
    s = Scene()
    s.add(Object(plane((0.0, 1.0, 0.0), -1.0)).material(Material.diffuse(hex_color(0x999999))))
    s.add(Object(polygon([(-5.5, -1.0, -5.0), (5.5, -1.0, -5.0), (5.5, 0.5, -5.0), (-5.5, 0.5, -5.0)]))
          .material(Material.diffuse(hex_color(0x8899AA))))
    of = [-1, -1]
    for i, (_, m) in enumerate(MATERIALS):
        if part is None or i % part[1] == part[0]:
            s.add(Object(shape(i, meshed)).material(m))
            of.append(i)
    if lit:
        s.add(Light.Ambient((0.04, 0.04, 0.05)))
        s.add(Light.Point((30.0, 28.0, 25.0), (3.0, 4.0, 3.5)))
        s.add(Light.Directional((0.4, 0.4, 0.5), (0.3, -1.0, -0.2)))
    s.add(Light.Object(Object(sphere().scale((0.3, 0.3, 0.3)).translate((-4.0, 0.4, 2.6)))
                       .material(Material.light((1.0, 0.9, 0.8), 60.0))))
    return s, tuple(of)


def camera(inside=False):
    """outside: all rows in view; inside: at the centre of the transparent cube INSIDE, so that first hits are exits —
    wide enough to see five of its faces, some at grazing angles"""
    if inside:
        x, y, z = place(INSIDE)
        return Camera.look_at((x, y, z), (x - 1.0, y + 0.35, z + 2.0), (0.0, 1.0, 0.0), 2.2)
    return Camera.look_at((0.0, 5.2, 6.4), (0.0, -0.8, -1.5), (0.0, 1.0, 0.0), 1.02)


def params(sample=0, samples=None, flags=0):
    return make_params(FRAME["width"], FRAME["height"], FRAME["bounces"], FRAME["samples"] if samples is None else samples,
                       seed=FRAME["seed"], sample_index_base=sample, flags=flags)


# ---- one path from the oracle's per-function entry points
class Chain:
    """a scene's materials and lights lowered once, and one shading step through oracle_illuminate, oracle_sample_f
    and oracle_bsdf"""

    def __init__(self, scene):
        from oracle import oracle_ffi
        self.L = oracle_ffi.lib()
        self.scene = scene
        self.materials = [o._material.lower() for o in scene.objects]
        self.keep = []
        self.lights = []
        for l in scene.lights:
            rec = _abi.RptLight()
            l.lower_into(rec, self.keep)
            self.lights.append(rec)
        self._n, self._wo, self._wi, self._pos = ((C.c_double * 3)() for _ in range(4))
        self._out3, self._out7 = (C.c_double * 3)(), (C.c_double * 7)()

    def step(self, obj, normal, position, direction, seed, stream, sample, draw, bounce=True, osc=None):
        """at a hit of object `obj` by a ray of `direction`, the stream at `draw`: the lights' draws, then sample_f and
        bsdf -> (some, wi, 1/pdf, f, |wi.n|, the draw sample_f ended at, A); bounce=False: a path's vertex at its last
        depth, where only the lights draw.  A, with an OracleScene for the shadow rays (else None): the vertex's own
        radiance, emittance * colour + sample_lights (renderer.rs:156-158, 177-204) in the oracle's operation order"""
        d = np.asarray(direction, dtype=np.float64)
        with np.errstate(all="ignore"):  # (IEEE throughout: a NaN direction gives a NaN wo, as in the oracle)
            length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])  # dot's order; normalize = self / self.norm()
            self._wo[:] = [float(x) for x in -(d / length)]
        self._n[:] = [float(x) for x in normal]
        self._pos[:] = [float(x) for x in position]
        m = self.materials[obj]
        n = self._n
        dr = C.c_uint32(int(draw))
        A = None
        if osc is not None:
            color = np.array(m.color[:])
            A = np.float64(m.emittance) * color
            lights = np.zeros(3)
        for rec in self.lights:
            if rec.kind == _abi.RPT_LIGHT_AMBIENT:  # (an ambient light takes no draw)
                if osc is not None:
                    lights = lights + np.array(rec.color[:]) * color
                continue
            rc = self.L.oracle_illuminate(C.byref(rec), self._pos, C.c_uint64(seed), C.c_uint32(stream), C.c_uint64(sample),
                                          C.byref(dr), self._out7)
            assert rc == 0
            if osc is not None:
                intensity, wl, dist = np.array(self._out7[0:3]), self._out7[3:6], self._out7[6]
                t, _, hit = osc.closest_hit(self._pos[:], wl)
                if hit[0] < 0 or t[0] > dist:
                    self.L.oracle_bsdf(C.byref(m), self._n, self._wo, (C.c_double * 3)(*wl), self._out3)
                    with np.errstate(all="ignore"):
                        lights = lights + (np.array(self._out3[:]) * intensity) * np.float64((wl[0] * n[0] + wl[1] * n[1]) + wl[2] * n[2])
        if osc is not None:
            A = A + lights
        if not bounce:
            return False, None, 0.0, None, 0.0, dr.value, A
        pdf = C.c_double(0.0)
        some = self.L.oracle_sample_f(C.byref(m), self._n, self._wo, C.c_uint64(seed), C.c_uint32(stream), C.c_uint64(sample),
                                      C.byref(dr), self._wi, C.byref(pdf))
        if not some:
            return False, None, 0.0, None, 0.0, dr.value, A
        wi = np.array(self._wi[:])
        self.L.oracle_bsdf(C.byref(m), self._n, self._wo, self._wi, self._out3)
        f = np.array(self._out3[:])
        abs_cos = abs((wi[0] * n[0] + wi[1] * n[1]) + wi[2] * n[2])
        with np.errstate(all="ignore"):
            inv_pdf = float(np.float64(1.0) / np.float64(pdf.value))
        return True, wi, inv_pdf, f, float(abs_cos), dr.value, A

    def escape(self, direction):
        """the environment's colour for a ray that leaves the scene"""
        from oracle import oracle_ffi
        return oracle_ffi.env_color(self.scene.environment, direction)


_chains = {}


def chain(scene):
    if id(scene) not in _chains:
        _chains[id(scene)] = (scene, Chain(scene))  # (the scene is kept: its id stays its own)
    return _chains[id(scene)][1]


def oracle_path(osc, scene, o, d, stream, sample, first_draw, seed, B):
    """One path of at most B bounces along the ray (o, d), the Philox stream (seed, stream, sample) at first_draw, from
    the oracle's per-function entry points only.  Per depth: osc.closest_hit; position = o + t * d (Ray::at, shape.rs:59);
    wo = -normalize(d); oracle.illuminate once per non-ambient light in scene order (sample_lights' only draws);
    oracle.sample_f at the draw that results; oracle.bsdf; |dot(wi, n)|.
    -> (vertices, length): per depth (object, normal, position, direction, draw_at_vertex, f, 1/pdf, abs_cos, A); a path's
    last vertex — an escape (object -1), depth B, or a hit where sample_f gave None — has f = 0, 1/pdf = 0, abs_cos = 0.
    A is the vertex's own radiance, trace_sample's A_k: the environment's colour at an escape, else the emission and every
    light's share from illuminate's result, a shadow closest_hit and bsdf, in the order of sample_lights"""
    ch = chain(scene)
    o, d = np.array(o, dtype=np.float64), np.array(d, dtype=np.float64)
    draw = int(first_draw)
    zero = np.zeros(3)
    out = []
    for depth in range(B + 1):
        t, n, obj = osc.closest_hit(o, d)
        obj = int(obj[0])
        if obj < 0:
            out.append((-1, zero, zero, d, draw, zero, 0.0, 0.0, ch.escape(d)))
            break
        pos = o + t[0] * d
        some, wi, inv_pdf, f, abs_cos, after, A = ch.step(obj, n[0], pos, d, seed, stream, sample, draw, bounce=depth < B, osc=osc)
        if not some:
            out.append((obj, n[0], pos, d, draw, zero, 0.0, 0.0, A))
            break
        out.append((obj, n[0], pos, d, draw, f, inv_pdf, abs_cos, A))
        o, d, draw = pos, wi, after
    return out, len(out)


# ---- rays no camera makes
PROBE_SAMPLES = 2


def _to_world(i, point, vector):
    m = np.array(shape(i).transform_m, dtype=np.float64).reshape(4, 4).T  # (column-major)
    return m[:3, :3] @ point + m[:3, 3], m[:3, :3] @ vector


@functools.lru_cache(maxsize=None)
def probe_rays():
    """Caller rays for the lit scene -> (o, d, streams, kind): camera rays with directions of length 3.0 and 1e-3; origins
    inside every transparent cube; rays 1e-6 rad off a face's plane of every cube from outside and of every transparent
    cube from inside (they start 1e-7 of the cube's size off the face and meet it after a tenth of its size); tangent
    rays 1e-10 radii under the surface of every transparent sphere.  Stream ids are scattered over 32 bits — but where an
    inside grazing ray's material has an index above 1.0, the id is the first one (searched with the oracle alone)
    under which sample_f at the ray's first vertex, sample 0, first_draw 0, is None: the window is 4.5e-4 wide at
    index 1.0000001, which no camera path of the frames meets.  (At index exactly 1.0 there is no None to find:
    sin2_ti = |wo - h (h.wo)|^2 <= |wo|^2, above 1.0 only by a rounding of the last bit.)"""
    from oracle import oracle_ffi
    rs = np.random.RandomState(0x9A2E)
    sc, of = scene(True)
    osc = oracle_ffi.OracleScene(sc)
    ch = chain(sc)
    o, d, streams, kind = [], [], [], []

    def add(oo, dd, what, stream=None):
        o.append(oo), d.append(dd), kind.append(what)
        streams.append(int(rs.randint(0, 2 ** 32, dtype=np.uint64)) if stream is None else stream)

    p = params()
    cam = camera(False)
    for k, pix in enumerate(range(7, p.width * p.height, 13)):  # 148 camera rays, stretched and shrunk
        oo, dd = oracle_ffi.camera_ray(cam, p, pix % p.width, pix // p.width, 0)
        add(oo, dd * (3.0 if k % 2 else 1e-3), "scaled")
    g = 1e-6
    for i, (_, m) in enumerate(MATERIALS):
        if is_cube(i):
            for k in range(2):  # from outside, towards face +x / -y at 1e-6 rad
                phi = rs.uniform(0.0, 2.0 * math.pi)
                u, v = rs.uniform(-0.3, 0.3, 2)
                axis = k  # 0: the face x = +0.5, 1: the face y = -0.5
                sign = 1.0 if k == 0 else -1.0
                pl = np.array([u, v, 0.0])
                dl = np.array([math.cos(g) * math.cos(phi), math.cos(g) * math.sin(phi), 0.0]) * 0.9
                pl = np.insert(pl[:2], axis, sign * (0.5 + 1e-7))
                dl = np.insert(dl[:2], axis, -sign * math.sin(g))
                add(*_to_world(i, pl, dl), "outside grazing")
        if not m.transparent:
            continue
        for k in range(4):
            if is_cube(i):
                add(*_to_world(i, rs.uniform(-0.45, 0.45, 3), rs.standard_normal(3)), "inside")
        for k in range(4):
            if is_cube(i):
                phi = rs.uniform(0.0, 2.0 * math.pi)
                axis, sign = k % 3, (1.0 if k < 2 else -1.0)
                u, v = rs.uniform(-0.3, 0.3, 2)
                pl = np.insert(np.array([u, v]), axis, sign * (0.5 - 1e-7))
                dl = np.insert(np.array([math.cos(g) * math.cos(phi), math.cos(g) * math.sin(phi)]) * 0.9, axis, sign * math.sin(g))
            else:
                u = rs.standard_normal(3)
                u /= np.linalg.norm(u)
                t = np.cross(u, rs.standard_normal(3))
                pl, dl = (1.0 - 1e-10) * u, t / np.linalg.norm(t)
            oo, dd = _to_world(i, pl, dl)
            stream = None
            if k == 0 and m.index > 1.0:
                t0, n0, obj0 = osc.closest_hit(oo, dd)
                assert of[int(obj0[0])] == i, (i, k)
                pos = oo + t0[0] * dd
                for stream in range(1 << 20):
                    if not ch.step(int(obj0[0]), n0[0], pos, dd, FRAME["seed"], stream, 0, 0)[0]:
                        break
                else:
                    raise AssertionError("no stream under which sample_f is None for %s" % MATERIALS[i][0])
            add(oo, dd, "inside grazing", stream)
    out = np.array(o), np.array(d), np.array(streams, dtype=np.uint32), tuple(kind)
    for a in out[:3]:
        a.setflags(write=False)
    return out


# ---- what a set of paths covers, from the oracle's records alone
def records(osc, cam, p):
    """OracleScene.trace_sample of every pixel and sample of p -> (rec [paths][B + 1][8], len [paths]), pixel-major"""
    n = p.width * p.height * p.iterations
    rec = np.zeros((n, p.max_bounces + 1, 8))
    length = np.zeros(n, dtype=np.int64)
    k = 0
    for y in range(p.height):
        for x in range(p.width):
            for s in range(p.iterations):
                _, r = osc.trace_sample(cam, p, x, y, p.sample_index_base + s)
                rec[k, :len(r)] = r
                length[k] = len(r)
                k += 1
    return rec, length


def suffixes(rec, length):
    """the estimator's fold over trace_sample's records -> L [paths][B + 1][3], the suffix value at every vertex"""
    n, V, _ = rec.shape
    L = np.zeros((n, V, 3))
    with np.errstate(all="ignore"):
        for d in range(V - 1, -1, -1):
            last, inner = length - 1 == d, length - 1 > d
            L[last, d] = rec[last, d, :3]
            if d + 1 < V:
                ind = (rec[:, d, 6, None] * (rec[:, d, 3:6] * L[:, d + 1])) * rec[:, d, 7, None]
                L[inner, d] = (rec[:, d, :3] + np.fmin(ind, 100.0))[inner]
    return L


def census(rec, length):
    """-> (inner vertices, those whose suffix L_{d+1} is +-0 in every channel, those with a non-finite f, 1/pdf or |cos|)"""
    L = suffixes(rec, length)
    V = rec.shape[1]
    inner = np.arange(V)[None, :] < length[:, None] - 1
    zero = np.zeros_like(inner)
    zero[:, :-1] = (L[:, 1:] == 0.0).all(axis=2)
    nonfinite = ~np.isfinite(rec[:, :, 3:8]).all(axis=2)
    return int(inner.sum()), int((inner & zero).sum()), int((inner & nonfinite).sum())


def oracle_vertices(osc, scene, o, d, streams, samples, base, first_draw, seed, B):
    """oracle_path of every (ray, sample) in trace_vertices' layout -> a dict of arrays (n, samples[, B + 1[, 3]]):
    length, object, normal, position, direction, draw, radiance, bsdf, inv_pdf, abs_cos, filled behind a path's end as
    the call fills"""
    n = len(o)
    v = {"length": np.zeros((n, samples), dtype=np.uint32), "object": np.full((n, samples, B + 1), -1, dtype=np.int32),
         "draw": np.zeros((n, samples, B + 1), dtype=np.uint32), "inv_pdf": np.zeros((n, samples, B + 1)),
         "abs_cos": np.zeros((n, samples, B + 1))}
    for k in ("normal", "position", "direction", "bsdf", "radiance"):
        v[k] = np.zeros((n, samples, B + 1, 3))
    for i in range(n):
        for s in range(samples):
            path, length = oracle_path(osc, scene, o[i], d[i], int(streams[i]), base + s, first_draw, seed, B)
            v["length"][i, s] = length
            for k, (obj, nrm, pos, dirn, draw, f, inv_pdf, abs_cos, A) in enumerate(path):
                v["object"][i, s, k], v["normal"][i, s, k], v["position"][i, s, k], v["direction"][i, s, k] = obj, nrm, pos, dirn
                v["draw"][i, s, k], v["bsdf"][i, s, k], v["inv_pdf"][i, s, k], v["abs_cos"][i, s, k] = draw, f, inv_pdf, abs_cos
                v["radiance"][i, s, k] = A
    for a in v.values():
        a.setflags(write=False)
    return v


def outcomes(v, of, B):
    """per material index: [inner vertices, reflections (wi on wo's side), transmissions, hits before depth B where the
    path ended by itself (sample_f gave None)] over the vertices of an oracle_vertices / trace_vertices result"""
    out = {i: [0, 0, 0, 0] for i in range(len(MATERIALS))}
    length, obj = v["length"].astype(np.int64), v["object"]
    depth = np.arange(B + 1)[None, None, :]
    inner = depth < length[:, :, None] - 1
    ended = (depth == length[:, :, None] - 1) & (depth < B) & (obj >= 0)
    with np.errstate(all="ignore"):
        wo_side = -(v["direction"] * v["normal"]).sum(axis=3) > 0.0
        wi_side = np.zeros_like(wo_side)
        wi_side[:, :, :-1] = (v["direction"][:, :, 1:] * v["normal"][:, :, :-1]).sum(axis=3) > 0.0
    material = np.where(obj >= 0, np.array(of)[np.maximum(obj, 0)], -1)
    for i in out:
        mine = material == i
        out[i] = [int((mine & inner).sum()), int((mine & inner & (wo_side == wi_side)).sum()),
                  int((mine & inner & (wo_side != wi_side)).sum()), int((mine & ended).sum())]
    return out
