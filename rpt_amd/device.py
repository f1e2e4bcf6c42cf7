"""Thin object wrapper over the C ABI (include/rpt_gpu.h): scene upload, the render-batch
hot path, the closest-hit kernel and the accounting.  Everything here calls into
`librptgpu.so`; nothing is computed in Python."""
import ctypes as C

import numpy as np

from . import _abi, _marshal
from .scene import geometry_mismatch, geometry_snapshot
from .shape import XF_WORDS, KdTree, Transformed, lower_shapes


def make_params(width, height, max_bounces, iterations, exposure_value=0.0, seed=0x52505447,
                sample_index_base=0, tile=(32, 8), part=(0, 1),
                precision=_abi.RPT_PRECISION_F64_STRICT, flags=0, collective=_abi.RPT_COLLECTIVE_DEFAULT):
    p = _abi.RptRenderParams()
    p.collective = int(collective)
    p.width, p.height, p.max_bounces, p.iterations = int(width), int(height), int(max_bounces), int(iterations)
    p.exposure_value = float(exposure_value)
    p.seed, p.sample_index_base = int(seed), int(sample_index_base)
    p.tile_width, p.tile_height = int(tile[0]), int(tile[1])
    p.part_index, p.part_count = int(part[0]), int(part[1])
    p.precision_mode, p.flags = int(precision), int(flags)
    return p


def scene_options(**fields):
    """RptSceneOptions with the library's defaults (rptgpu_scene_options_default) and the given fields set."""
    o = _abi.RptSceneOptions()
    _abi.load_library().rptgpu_scene_options_default(C.byref(o))
    known = {name for name, _ in _abi.RptSceneOptions._fields_}
    for k, v in fields.items():
        if k not in known or k in ("struct_size", "_reserved0"):
            raise TypeError("RptSceneOptions has no field %r" % k)
        setattr(o, k, v)
    return o


def _lower_camera(camera):
    """a Camera lowered; an RptCamera as it is"""
    return camera.lower() if hasattr(camera, "lower") else camera


def device_count():
    lib = _abi.load_library()
    n = C.c_int(0)
    _abi.check(lib.rptgpu_device_count(C.byref(n)))
    return n.value


class PathVertices:
    """GpuScene.trace_vertices' result: `channels` (the RPT_VERTEX_* bits that were asked for) and one attribute per channel
    — length, t, normal, object, position, direction, draw, radiance, bsdf, inv_pdf, abs_cos, rgb — holding its array (numpy,
    or torch on the device), or None when the channel was not named."""
    NAMES = ("length", "t", "normal", "object", "position", "direction", "draw", "radiance", "bsdf", "inv_pdf", "abs_cos", "rgb")
    __slots__ = ("channels",) + NAMES

    def __init__(self, channels):
        self.channels = int(channels)
        for name in self.NAMES:
            setattr(self, name, None)

    def arrays(self):
        """{name: array} of the channels that were named"""
        return {name: getattr(self, name) for name in self.NAMES if getattr(self, name) is not None}


class GpuScene:
    """Owns one `rptgpu_scene*` (device-resident flattened scene + kd-trees)."""

    def __init__(self, scene, device=0, **options):
        """options: fields of RptSceneOptions (include/rpt_gpu.h) by name, e.g. GpuScene(scene, 0, sort_rays=0,
        deep_depth=1); the rest keep their defaults.  RPTGPU_* environment variables still override."""
        self.lib = _abi.load_library()
        desc, keep = scene.lower()
        h = C.c_void_p()
        if options:
            o = scene_options(**options)
            _abi.check(self.lib.rptgpu_scene_create_opts(C.byref(desc), int(device), C.byref(o), C.byref(h)))
        else:
            _abi.check(self.lib.rptgpu_scene_create(C.byref(desc), int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)
        self._geometry = geometry_snapshot(scene)  # what update() compares a new scene against

    # ---- live updates (rptgpu_scene_set_objects / _lights): new placements and materials, same geometry.  Afterwards
    # every result equals that of a GpuScene made from the updated scene; the workspace and DeviceBuffers stay.
    def set_objects(self, indices, objects):
        """Object indices[k] := objects[k] (a Python Object): its Transformed fields and its material.  The shape's
        geometry is not read; its kind and whether it is Transformed must be the creation's."""
        indices, objects = list(indices), list(objects)
        if len(indices) != len(objects):
            raise ValueError("set_objects: %d indices for %d objects" % (len(indices), len(objects)))
        keep = []
        arr = (_abi.RptObject * max(1, len(objects)))()
        for k, o in enumerate(objects):
            o.lower_into(arr[k], keep)
        idx = (C.c_uint32 * max(1, len(indices)))(*[int(i) for i in indices])
        _abi.check(self.lib.rptgpu_scene_set_objects(self.handle, len(objects), idx, arr), self.handle)

    def set_lights(self, indices, lights):
        """Light indices[k] := lights[k] (a Python Light): colour and vector, or a Light::Object's placement and
        material.  The kind must be the creation's; a Light::Object's shape geometry is not read."""
        indices, lights = list(indices), list(lights)
        if len(indices) != len(lights):
            raise ValueError("set_lights: %d indices for %d lights" % (len(indices), len(lights)))
        keep = []
        arr = (_abi.RptLight * max(1, len(lights)))()
        for k, l in enumerate(lights):
            l.lower_into(arr[k], keep)
        idx = (C.c_uint32 * max(1, len(indices)))(*[int(i) for i in indices])
        _abi.check(self.lib.rptgpu_scene_set_lights(self.handle, len(lights), idx, arr), self.handle)

    def update(self, scene):
        """Push every object and light of `scene`, a Scene with the geometry of the one this handle was made from (the
        next frame of an animation).  ValueError, naming the first mismatch, when the counts, the environment or any
        shape's geometry differ (scene.geometry_mismatch): those need a new GpuScene."""
        why = geometry_mismatch(self._geometry, scene)
        if why:
            raise ValueError("GpuScene.update: %s; a new GpuScene is needed" % why)
        self.set_objects(range(len(scene.objects)), scene.objects)
        self.set_lights(range(len(scene.lights)), scene.lights)
        self._geometry = geometry_snapshot(scene)  # (the same geometry: the newer objects make the identity checks hit)

    # ---- a deforming mesh (rptgpu_scene_set_mesh[_device]): new triangles for one mesh, the count unchanged.  The mesh's
    # records and tree are rebuilt on the device; afterwards every result equals that of a GpuScene made from the scene in
    # which that mesh has the new triangles.  update()'s geometry snapshot is the creation's: update() keeps comparing
    # placements against the scene the handle was made from.
    def set_mesh(self, index, triangles):
        """Object `index` (a top-level Mesh) gets `triangles`: (n, 18) float64 — v1 v2 v3 n1 n2 n3 per row, n the mesh's
        count at creation — as a numpy array, or as a contiguous torch tensor on the handle's device, which is read there
        after torch's current stream (no triangle goes through the host).  Other shapes and dtypes raise here."""
        index = int(index)
        if index < 0:
            raise ValueError("set_mesh: object index %d is negative" % index)
        m = _marshal.pick(self.device, triangles)
        rows = m.rows(triangles, 18, "set_mesh", "triangles")
        self._call("rptgpu_scene_set_mesh", m, index, int(rows.shape[0]), m.pointer(rows, C.POINTER(_abi.RptTriangle)))

    # ---- a group whose children move (rptgpu_scene_set_group[_device]): new placements for the children of one
    # KdTree of spheres and cubes, the count, the kinds and which children are Transformed unchanged.  The children's
    # records and the group's tree are rebuilt on the device; afterwards every result equals that of a GpuScene made
    # from the scene in which the group has the new children.  update()'s geometry snapshot stays the creation's.
    def set_group(self, index, children):
        """Object `index` (a top-level KdTree of shapes) gets new placements for its children: a sequence of Python
        shapes (child i of the kind it had at creation, Transformed if it was), or their RptTransform records as an
        (n, 51) float64 array (rpt_amd.transform_records) — numpy, or a contiguous torch tensor on the handle's device,
        which is read there after torch's current stream.  Other shapes, dtypes and devices raise here."""
        index = int(index)
        if index < 0:
            raise ValueError("set_group: object index %d is negative" % index)
        m = _marshal.pick(self.device, children)
        if m.suffix:  # records on the device: the library reads them there
            rows = m.rows(children, XF_WORDS, "set_group", "transform records")
            return self._call("rptgpu_scene_set_group", m, index, int(rows.shape[0]), m.pointer(rows, None))
        if isinstance(children, np.ndarray):
            rows = m.rows(children, XF_WORDS, "set_group", "transform records")
            arr, n = self._creation_children(index)
            if n != rows.shape[0]:
                raise ValueError("set_group: %d transform records for the %d children of object %d" % (rows.shape[0], n, index))
            if n:  # the records into the xf fields of the creation's children (kinds and `transformed` as they were)
                raw = np.frombuffer(arr, dtype=np.uint8).reshape(-1, C.sizeof(_abi.RptShape))[:n]
                at = _abi.RptShape.xf.offset
                raw[:, at:at + 8 * XF_WORDS] = rows.view(np.uint8).reshape(n, 8 * XF_WORDS)
        else:
            children = list(children)
            keep = []
            arr, n = lower_shapes(children, keep), len(children)
        self._call("rptgpu_scene_set_group", m, index, n, arr)

    def _creation_children(self, index):
        """the children of object `index` as lowered at creation (cached: set_group writes new records into it)"""
        cache = self.__dict__.setdefault("_group_children", {})
        if index not in cache:
            objects = self._geometry.objects
            shape = objects[index].shape if index < len(objects) else None
            if isinstance(shape, Transformed):
                shape = shape.shape
            if not isinstance(shape, KdTree) or shape.objects is None:
                raise ValueError("set_group: object %d is not a KdTree of shapes" % index)
            keep = []
            cache[index] = (lower_shapes(shape.objects, keep), len(shape.objects), keep)
        return cache[index][:2]

    def options(self):
        """The options the handle runs with (defaults, the caller's, environment overrides) as a dict."""
        o = _abi.RptSceneOptions()
        o.struct_size = C.sizeof(_abi.RptSceneOptions)  # ABI v7: the caller says how large ITS struct is
        _abi.check(self.lib.rptgpu_scene_get_options(self.handle, C.byref(o)), self.handle)
        return {name: getattr(o, name) for name, _ in _abi.RptSceneOptions._fields_ if not name.startswith("_")}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rptgpu_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_batch(self, camera, params):
        """Renderer::sample's output: (H*W, 3) float64 means, row-major, top row first."""
        out = np.empty((params.height * params.width, 3), dtype=np.float64)
        cam = _lower_camera(camera)
        code = self.lib.rptgpu_render_batch(self.handle, C.byref(cam), C.byref(params),
                                            out.ctypes.data_as(C.POINTER(C.c_double)))
        _abi.check(code, self.handle)
        return out

    def render_batch_device(self, camera, params, d_ptr, out_is_f32=False, stream=None):
        cam = _lower_camera(camera)
        code = self.lib.rptgpu_render_batch_device(self.handle, C.byref(cam), C.byref(params),
                                                   C.c_void_p(d_ptr), 1 if out_is_f32 else 0,
                                                   C.c_void_p(stream or 0))
        _abi.check(code, self.handle)

    # ---- multi-GPU: the library's own RCCL communicator (include/rpt_gpu.h) ----
    @staticmethod
    def comm_unique_id():
        """rank 0: the 128-byte id every rank passes to comm_init (hand it over any side channel)"""
        lib = _abi.load_library()
        buf = (C.c_uint8 * _abi.RPTGPU_UNIQUE_ID_BYTES)()
        _abi.check(lib.rptgpu_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        buf = (C.c_uint8 * _abi.RPTGPU_UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _abi.check(self.lib.rptgpu_comm_init(self.handle, int(rank), int(world), buf), self.handle)

    def comm_destroy(self):
        _abi.check(self.lib.rptgpu_comm_destroy(self.handle), self.handle)

    def render_batch_reduce(self, camera, params, root=0, out=None):
        """Renderer::sample on every rank: this rank's tiles, the owned pixels gathered on `root` over RCCL
        (params.collective = RPT_COLLECTIVE_REDUCE: ncclReduce(sum) of zero-filled frames), result in host memory on root.  `out`: float32 array of width*height*3 (allocated if None on root)."""
        cam = _lower_camera(camera)
        if out is None:
            out = np.empty(params.height * params.width * 3, dtype=np.float32)
        code = self.lib.rptgpu_render_batch_reduce(self.handle, C.byref(cam), C.byref(params), int(root),
                                                   out.ctypes.data_as(C.POINTER(C.c_float)))
        _abi.check(code, self.handle)
        return out

    def render_batch_emulate_ranks(self, camera, params, world, out=None):
        """Diagnostics: the frame as `world` ranks' gather would assemble it, on this one GPU (include/rpt_gpu.h)."""
        cam = _lower_camera(camera)
        if out is None:
            out = np.empty(params.height * params.width * 3, dtype=np.float32)
        code = self.lib.rptgpu_render_batch_emulate_ranks(self.handle, C.byref(cam), C.byref(params), int(world),
                                                          out.ctypes.data_as(C.POINTER(C.c_float)))
        _abi.check(code, self.handle)
        return out

    # ---- the array calls.  Each is one body written against a backend of _marshal.py — _marshal.HOST for numpy arrays, the
    # device backend for torch tensors on the handle's device —, which checks the arrays, allocates the results and says
    # in which form the symbol takes a pointer; _call appends the backend's suffix and stream argument.
    def _call(self, name, m, *args):
        """rptgpu_<name>, or for the device backend rptgpu_<name>_device with the stream behind the arguments"""
        _abi.check(getattr(self.lib, name + m.suffix)(self.handle, *args, *m.stream_args()), self.handle)

    _RAYS = ("origins", "dirs", "{a} origins for {b} directions")
    _POINTS = ("positions", "normals", "{b} normals for {a} positions")

    @staticmethod
    def _pair(m, a, b, who, names, coerce=False):
        """two (n, 3) float64 arrays of one length, named by _RAYS or _POINTS -> (n, the two as the backend takes them)"""
        a, b = m.vectors(a, who, names[0], coerce), m.vectors(b, who, names[1], coerce)
        n = int(a.shape[0])
        if int(b.shape[0]) != n:
            raise ValueError(who + ": " + names[2].format(a=n, b=int(b.shape[0])))
        return n, a, b

    def closest_hit(self, origins, dirs, precision=_abi.RPT_PRECISION_F64_STRICT):
        m = _marshal.HOST  # (numpy only)
        # the call's contract: anything that reshapes to (n, 3) doubles, and the directions' count is the library's to check
        o, d = m.vectors(origins, "closest_hit", "origins", coerce=True), m.vectors(dirs, "closest_hit", "dirs", coerce=True)
        n = len(o)
        t, nrm, obj = (m.result(None, shape, dtype, "closest_hit", "") for shape, dtype in
                       (((n,), np.float64), ((n, 3), np.float64), ((n,), np.int32)))
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_closest_hit", m, n, m.pointer(o, PD), m.pointer(d, PD), int(precision), m.pointer(t, PD),
                   m.pointer(nrm, PD), m.pointer(obj, C.POINTER(C.c_int32)))
        return t, nrm, obj

    def trace_rays(self, origins, dirs, max_bounces, samples=1, seed=0x52505447, sample_index_base=0, streams=None,
                   first_draw=0, exposure_value=0.0, flags=0, out=None):
        """Path-traced radiance along the caller's rays (rptgpu_trace_rays) -> (n, 3) float64: per ray the
        mean of `samples` paths of at most max_bounces bounces, times 2^exposure_value.  origins, dirs: (n, 3) float64, the
        directions unit vectors (they are used as given).  streams: (n,) 32-bit stream ids, default the rays' indices; ray
        i's random numbers are those of (seed, streams[i], sample_index_base + s) from draw first_draw on, so its result
        does not depend on the rays around it.  numpy arrays go through host memory; torch tensors on the handle's device
        are read where they lie (rptgpu_trace_rays_device) and the result is `out` or a new tensor there."""
        q = _abi.RptRayQuery()
        q.struct_size = C.sizeof(_abi.RptRayQuery)
        q.max_bounces, q.iterations, q.first_draw = int(max_bounces), int(samples), int(first_draw)
        q.exposure_value, q.seed, q.sample_index_base = float(exposure_value), int(seed), int(sample_index_base)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        m = _marshal.pick(self.device, origins, dirs)
        # the call's contract: rays of any dtype that reshape to (n, 3), and ids of any dtype and shape that flatten to n
        n, o, d = self._pair(m, origins, dirs, "trace_rays", self._RAYS, coerce=True)
        ids = m.stream_ids(streams, n, "trace_rays", "rays", strict=False)
        # (no room behind `out`: with n = 0 the library gets the address numpy or torch give, NULL for an empty tensor)
        out = m.result(out, (n, 3), np.float64, "trace_rays", "out")
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_trace_rays", m, n, m.pointer(o, PD), m.pointer(d, PD), m.pointer(ids, C.POINTER(C.c_uint32)),
                   C.byref(q), m.pointer(out, PD))
        return out

    def bake_probes(self, positions, normals=None, *, kind, samples, max_bounces, seed, sample_index_base=0, streams=None,
                    flags=0, out=None):
        """Light probes baked on the device (rptgpu_bake_probes): per probe `samples` directions from the
        Philox stream, one path of at most max_bounces bounces along each.  kind = RPT_PROBE_SH9 -> (n, 9, 3) float64, the
        radiance around positions[i] in the real spherical harmonics of bands 0-2 (rpt_amd.sh9_basis' order);
        RPT_PROBE_IRRADIANCE -> (n, 3), the irradiance of a surface at positions[i] with normal normals[i].  positions,
        normals: (n, 3) float64 (normals only with RPT_PROBE_IRRADIANCE).  streams: (n,) 32-bit stream ids, default the
        probes' indices; probe i's random numbers are those of (seed, streams[i], sample_index_base + k), so its result does
        not depend on the probes around it.  numpy arrays go through host memory; torch tensors on the handle's device are
        read where they lie (rptgpu_bake_probes_device) and the result is `out` or a new tensor there."""
        kind = int(kind)
        if kind not in (_abi.RPT_PROBE_SH9, _abi.RPT_PROBE_IRRADIANCE):
            raise ValueError("bake_probes: kind must be RPT_PROBE_SH9 or RPT_PROBE_IRRADIANCE")
        if kind == _abi.RPT_PROBE_IRRADIANCE and normals is None:
            raise ValueError("bake_probes: RPT_PROBE_IRRADIANCE needs normals")
        if kind == _abi.RPT_PROBE_SH9 and normals is not None:
            raise ValueError("bake_probes: RPT_PROBE_SH9 takes no normals")
        q = _abi.RptProbeQuery()
        q.struct_size = C.sizeof(_abi.RptProbeQuery)
        q.kind, q.samples, q.max_bounces = kind, int(samples), int(max_bounces)
        q.seed, q.sample_index_base = int(seed), int(sample_index_base)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        tail = (9, 3) if kind == _abi.RPT_PROBE_SH9 else (3,)
        m = _marshal.pick(self.device, positions, normals)
        # the call's contract: (n, 3) float64 as they come, and ids that are one-dimensional and integer
        if normals is None:
            pos, nrm = m.vectors(positions, "bake_probes", "positions"), None
            n = int(pos.shape[0])
        else:
            n, pos, nrm = self._pair(m, positions, normals, "bake_probes", self._POINTS)
        ids = m.stream_ids(streams, n, "bake_probes", "probes", strict=True)
        out = m.result(out, (n,) + tail, np.float64, "bake_probes", "out")
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_bake_probes", m, n, m.pointer(pos, PD), m.pointer(nrm, PD), m.pointer(ids, C.POINTER(C.c_uint32)),
                   C.byref(q), m.pointer(out, PD))
        return out

    def occluded(self, origins, dirs, max_t=None, flags=0, out=None):
        """Is anything between the ray's origin and max_t along it?  (rptgpu_occluded) -> (n,) uint8, 1 =
        occluded: exactly `~(t > fmin(max_t, DBL_MAX))` with t = closest_hit's, found by the shadow-ray query (it stops at
        the first blocker).  origins, dirs: (n, 3) float64, used as given; max_t: (n,) float64 in units of the ray
        parameter, None = +inf for every ray.  numpy arrays go through host memory; torch tensors on the handle's device
        are read where they lie (rptgpu_occluded_device) and the result is `out` or a new tensor there."""
        q = _abi.RptVisibilityQuery()
        q.struct_size = C.sizeof(_abi.RptVisibilityQuery)
        q.precision_mode, q.flags, q.reserved = _abi.RPT_PRECISION_F64_STRICT, int(flags), 0
        m = _marshal.pick(self.device, origins, dirs)
        n, o, d = self._pair(m, origins, dirs, "occluded", self._RAYS)  # the call's contract: (n, 3) float64 as they come
        mt = m.scalars(max_t, n, "occluded", "max_t")
        out = m.result(out, (n,), np.uint8, "occluded", "out")
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_occluded", m, n, m.pointer(o, PD), m.pointer(d, PD), m.pointer(mt, PD), C.byref(q),
                   m.pointer(out, C.POINTER(C.c_uint8)))
        return out

    def bake_ao(self, positions, normals, *, samples, seed, max_distance=float("inf"), sample_index_base=0, streams=None,
                bent_normals=False, flags=0, out=None):
        """Ambient occlusion baked on the device (rptgpu_bake_ao): per point `samples` cosine-weighted
        directions about its normal from the Philox stream (RPT_PROBE_IRRADIANCE's), each a visibility query up to
        max_distance -> (n,) float64, the unoccluded fraction (1.0 = open); with bent_normals=True -> (ao, bent), bent (n, 3)
        the mean of the visible directions' sum over all `samples` (the unnormalised bent normal).  The rays start AT the
        positions (no offset: lift points off their surface yourself).  positions, normals: (n, 3) float64.  streams: (n,)
        32-bit stream ids, default the points' indices.  out: None, an (n,) array for ao, or with bent_normals a pair
        (ao, bent).  numpy arrays go through host memory; torch tensors on the handle's device are read where they lie
        (rptgpu_bake_ao_device) and the results are `out` or new tensors there."""
        q = _abi.RptAoQuery()
        q.struct_size = C.sizeof(_abi.RptAoQuery)
        q.samples, q.seed, q.sample_index_base = int(samples), int(seed), int(sample_index_base)
        q.max_distance, q.precision_mode, q.flags = float(max_distance), _abi.RPT_PRECISION_F64_STRICT, int(flags)
        out_ao, out_bent = (out if isinstance(out, (tuple, list)) else (out, None)) if out is not None else (None, None)
        if out_bent is not None and not bent_normals:
            raise ValueError("bake_ao: an output for bent normals without bent_normals=True")
        m = _marshal.pick(self.device, positions, normals)
        # the call's contract: (n, 3) float64 as they come, and ids that are one-dimensional and integer
        n, pos, nrm = self._pair(m, positions, normals, "bake_ao", self._POINTS)
        ids = m.stream_ids(streams, n, "bake_ao", "points", strict=True)
        out_ao = m.result(out_ao, (n,), np.float64, "bake_ao", "the output for ao")
        out_bent = m.result(out_bent, (n, 3), np.float64, "bake_ao", "the output for bent normals") if bent_normals else None
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_bake_ao", m, n, m.pointer(pos, PD), m.pointer(nrm, PD), m.pointer(ids, C.POINTER(C.c_uint32)),
                   C.byref(q), m.pointer(out_ao, PD), m.pointer(out_bent, PD))
        return (out_ao, out_bent) if bent_normals else out_ao

    def bake_direct(self, positions, normals, *, samples, seed, sample_index_base=0, streams=None, flags=0, out=None):
        """Direct light baked on the device (rptgpu_bake_direct): per point `samples` rounds of the
        renderer's next-event estimation — every non-ambient light of the scene sampled in scene order on the point's Philox
        stream, `intensity * (wi . n)` added where the light faces the normal and the shadow ray reaches it — -> (n, 3)
        float64, the mean: irradiance without the Lambertian 1/pi, so `bsdf * out` is a surface's direct term.  The rays
        start AT the positions (no offset: lift points off their surface yourself).  positions, normals: (n, 3) float64.
        streams: (n,) 32-bit stream ids, default the points' indices.  numpy arrays go through host memory; torch tensors on
        the handle's device are read where they lie (rptgpu_bake_direct_device) and the result is `out` or a new tensor
        there."""
        if not _abi.direct_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_bake_direct")
        q = _abi.RptDirectQuery()
        q.struct_size = C.sizeof(_abi.RptDirectQuery)
        q.samples, q.seed, q.sample_index_base = int(samples), int(seed), int(sample_index_base)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        m = _marshal.pick(self.device, positions, normals)
        n, pos, nrm = self._pair(m, positions, normals, "bake_direct", self._POINTS)
        ids = m.stream_ids(streams, n, "bake_direct", "points", strict=True)
        out = m.result(out, (n, 3), np.float64, "bake_direct", "out")
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_bake_direct", m, n, m.pointer(pos, PD), m.pointer(nrm, PD), m.pointer(ids, C.POINTER(C.c_uint32)),
                   C.byref(q), m.pointer(out, PD))
        return out

    def render_views(self, views, width, height, max_bounces, samples=1, seed=0x52505447, seed_stride=0,
                     sample_index_base=0, exposure_value=0.0, flags=0, out=None, seeds=None):
        """A batch of frames in one call (rptgpu_render_views) -> (n, height, width, 3): per pixel the mean
        of `samples` paths of at most max_bounces bounces, times 2^exposure_value.  views: a sequence of View (a camera
        under RPT_VIEW_PERSPECTIVE / _ORTHOGRAPHIC / _PANORAMA), Camera (perspective) or _abi.RptView.  View v renders with
        seed + v * seed_stride, and pixel p's random numbers are those of (that seed, p, sample_index_base + s): a
        perspective view is render_batch's frame of its camera, and no view depends on the views around it.  seeds: one
        seed per view instead (a sequence of ints or a numpy uint64 array of len(views); rptgpu_render_views_seeded) — view
        v renders exactly as with seed = seeds[v] and seed_stride = 0; not together with a non-zero seed_stride.  out: None or
        a C-contiguous float64 numpy array (the frames go through host memory), or a contiguous float64 / float32 torch
        tensor on the handle's device, which is written where it lies (rptgpu_render_views_device)."""
        n, arr, seed_arr, q = self._view_query("render_views", views, width, height, max_bounces, samples, exposure_value, seed,
                                               seed_stride, seeds, sample_index_base, flags)
        m = _marshal.pick(self.device, out)
        # the ABI's difference: the device symbols also write float32 frames and say which behind the address
        dtypes = (np.float64, np.float32) if m.suffix else np.float64
        out = m.result(out, (n, int(height), int(width), 3), dtypes, "render_views", "out")
        f32 = (1 if out.element_size() == 4 else 0,) if m.suffix else ()
        seeded = ("_seeded", seed_arr) if seed_arr is not None else ("",)
        self._call("rptgpu_render_views" + seeded[0], m, n, arr, C.byref(q), *seeded[1:], m.pointer(out, C.POINTER(C.c_double)),
                   *f32)
        return out

    def _view_query(self, who, views, width, height, max_bounces, samples, exposure_value, seed, seed_stride, seeds,
                    sample_index_base, flags):
        """the render_views* calls' common half -> (n, the lowered views, the lowered seeds or None, their RptViewQuery)"""
        views = list(views)
        arr = self._lower_views(views, who)
        seed_arr = self._lower_seeds(seeds, len(views), seed_stride, who)
        q = _abi.RptViewQuery()
        q.struct_size = C.sizeof(_abi.RptViewQuery)
        q.width, q.height, q.max_bounces, q.iterations = int(width), int(height), int(max_bounces), int(samples)
        q.exposure_value, q.seed, q.seed_stride = float(exposure_value), int(seed), int(seed_stride)
        q.sample_index_base, q.precision_mode, q.flags = int(sample_index_base), _abi.RPT_PRECISION_F64_STRICT, int(flags)
        return len(views), arr, seed_arr, q

    def first_hits(self, origins, dirs, channels=_abi.RPT_HIT_ALL, flags=0):
        """The first hit of each of the caller's rays (rptgpu_first_hits) -> a dict with one array per
        channel of `channels` (RPT_HIT_*): `t` (n,) float64 — closest_hit's, +inf on a miss —, `normal` (n, 3), `object`
        (n,) int32 (-1 on a miss), `position` (n, 3) = origin + t * dir on a hit and +0.0 on a miss, `albedo` (n, 3) = the
        hit object's material colour, +0.0 on a miss.  origins, dirs: (n, 3) float64, used as given.  numpy arrays go
        through host memory; torch tensors on the handle's device are read where they lie (rptgpu_first_hits_device) and
        the results are new tensors there."""
        q = _abi.RptHitQuery()
        q.struct_size, q.channels = C.sizeof(_abi.RptHitQuery), int(channels)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        return self._ray_records("first_hits", origins, dirs, q, _abi.RptHitArrays(), _marshal.HIT_CHANNELS)

    def hit_surface(self, origins, dirs, channels=_abi.RPT_SURFACE_ALL, flags=0):
        """The surface element behind the first hit of each of the caller's rays (rptgpu_hit_surface) -> a
        dict with one array per channel of `channels` (RPT_SURFACE_*): `t` (n,) float64 and `object` (n,) int32 —
        closest_hit's, to join on —, `child` (n,) int32 — the hit group's direct child in the caller's order, else -1 —,
        `primitive` (n,) int32 — the hit triangle's index in its mesh in the caller's order, else -1 —, `barycentric`
        (n, 3) float64 — the weights (u, v, w) of v1, v2, v3 as Triangle::intersect computed them, +0.0 without a
        triangle (rpt_amd.surface.interpolate takes the last two).  origins, dirs: (n, 3) float64, used as given.  numpy
        arrays go through host memory; torch tensors on the handle's device are read where they lie
        (rptgpu_hit_surface_device) and the results are new tensors there."""
        if not _abi.hit_surface_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_hit_surface")
        q = _abi.RptSurfaceQuery()
        q.struct_size, q.channels = C.sizeof(_abi.RptSurfaceQuery), int(channels)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        return self._ray_records("hit_surface", origins, dirs, q, _abi.RptSurfaceArrays(), _marshal.SURFACE_CHANNELS)

    _FILTERS = {"nearest": _abi.RPT_LOOKUP_NEAREST, "bilinear": _abi.RPT_LOOKUP_BILINEAR}

    def lookup_lightmap(self, origins, dirs, bindings, *, filter="bilinear", fallback=(0.0, 0.0, 0.0),
                        channels=_abi.RPT_LOOKUP_ALL, flags=0):
        """Baked lightmaps read back at the first hit of each of the caller's rays (rptgpu_lookup_lightmap) ->
        a dict with one array per channel of `channels` (RPT_LOOKUP_*): `t` (n,) float64 and `object` (n,) int32 —
        closest_hit's, to join on —, `binding` (n,) int32 — the index in `bindings` of the lightmap.Binding that names the
        hit object, -1 for a miss, an object nobody names, a mesh inside a group —, `covered` (n,) uint8, `uv` (n, 2) —
        the hit triangle's uvs under hit_surface's barycentrics, surface.interpolate's order — and `value` (n, 3): the
        map's texel there under `filter` ("nearest", or "bilinear": clamp to edge, taps that are not valid left out and
        the weights renormalised), a one-component map's scalar three times, `fallback` where the ray is not covered.
        origins, dirs: (n, 3) float64, used as given.  numpy arrays go through host memory; torch tensors on the
        handle's device — rays and every binding's arrays alike — are read where they lie
        (rptgpu_lookup_lightmap_device) and the results are new tensors there."""
        if not _abi.lightmap_lookup_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_lookup_lightmap")
        who = "lookup_lightmap"
        if filter not in self._FILTERS:
            raise ValueError('%s: filter must be "nearest" or "bilinear", not %r' % (who, filter))
        q = _abi.RptLookupQuery()
        q.struct_size, q.channels, q.filter = C.sizeof(_abi.RptLookupQuery), int(channels), self._FILTERS[filter]
        q.fallback = _abi.V3(*(float(x) for x in fallback))
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        bindings = list(bindings)
        m = _marshal.pick(self.device, origins, dirs, *(x for b in bindings for x in (b.uvs, b.map, b.valid)))
        recs, keep = self._lower_bindings(m, bindings, who)
        a = _abi.RptLookupArrays()
        a.struct_size, a.reserved = C.sizeof(a), 0
        n, o, d = self._pair(m, origins, dirs, who, self._RAYS)
        out = m.fill(a, _marshal.layout(_marshal.LOOKUP_CHANNELS, q.channels, (n,)), who)
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_lookup_lightmap", m, n, m.pointer(o, PD), m.pointer(d, PD), len(bindings), recs, C.byref(q), C.byref(a))
        del keep
        return out

    def render_views_lightmapped(self, views, width, height, bindings, *, samples=1, seed, seed_stride=0, sample_index_base=0,
                                 exposure_value=0.0, filter="bilinear", unbound_irradiance=(0.0, 0.0, 0.0), flags=0, out=None):
        """A batch of views shaded from baked lightmaps (rptgpu_render_views_lightmapped) -> (n, height, width,
        3) float64.  views, width, height, samples, seed, seed_stride, sample_index_base, exposure_value: render_views' —
        the ray of (view, pixel, sample) is exactly that call's.  Per sample a miss gives the environment's colour and a
        hit on an object of material m gives m.emittance * m.color + m.color / pi * I, with I lookup_lightmap's `value`
        under `filter` where the ray is covered and `unbound_irradiance` elsewhere; a pixel is the mean over its samples
        times 2^exposure_value.  bindings: lightmap.Binding records of numpy arrays — the frames then come through host
        memory — or of torch tensors on the handle's device, which are read where they lie and give a new tensor there
        (rptgpu_render_views_lightmapped_device; out="torch" asks for that form when there is no binding to tell)."""
        if not _abi.lightmap_lookup_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_render_views_lightmapped")
        who = "render_views_lightmapped"
        if filter not in self._FILTERS:
            raise ValueError('%s: filter must be "nearest" or "bilinear", not %r' % (who, filter))
        if out not in (None, "torch"):
            raise ValueError('%s: out must be None or "torch"' % who)
        n, arr, _, qv = self._view_query(who, views, width, height, 0, samples, exposure_value, seed, seed_stride, None,
                                         sample_index_base, flags)
        q = _abi.RptViewsLightmapQuery()
        q.struct_size, q.filter = C.sizeof(q), self._FILTERS[filter]
        q.unbound_irradiance = _abi.V3(*(float(x) for x in unbound_irradiance))
        bindings = list(bindings)
        m = _marshal._Device(self.device) if out == "torch" else \
            _marshal.pick(self.device, *(x for b in bindings for x in (b.uvs, b.map, b.valid)))
        recs, keep = self._lower_bindings(m, bindings, who)
        frames = m.result(None, (n, int(height), int(width), 3), np.float64, who, "out")
        self._call("rptgpu_render_views_lightmapped", m, n, arr, C.byref(qv), len(bindings), recs, C.byref(q),
                   m.pointer(frames, C.POINTER(C.c_double)))
        del keep
        return frames

    def _volume_call(self, name, who, a, b, names, volume, normal_bias, fallback, channels, flags):
        """sample_probe_volume's and lookup_probe_volume's one body: the query, the volume, the pair of (n, 3) inputs, the
        named channels' arrays -> the dict"""
        if not _abi.probe_volume_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export " + name)
        q = _abi.RptVolumeQuery()
        q.struct_size, q.channels, q.normal_bias = C.sizeof(q), int(channels), float(normal_bias)
        q.fallback = _abi.V3(*(float(x) for x in fallback))
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        m = _marshal.pick(self.device, a, b, volume.coeffs, volume.valid)
        rec, keep = self._lower_volume(m, volume, who)
        arrays = _abi.RptVolumeArrays()
        arrays.struct_size, arrays.reserved = C.sizeof(arrays), 0
        n, a, b = self._pair(m, a, b, who, names)
        out = m.fill(arrays, _marshal.layout(_marshal.VOLUME_CHANNELS, q.channels, (n,)), who)
        PD = C.POINTER(C.c_double)
        self._call(name, m, n, m.pointer(a, PD), m.pointer(b, PD), C.byref(rec), C.byref(q), C.byref(arrays))
        del keep
        return out

    def sample_probe_volume(self, positions, normals, volume, *, normal_bias=0.0, fallback=(0.0, 0.0, 0.0),
                            channels=_abi.RPT_VOLUME_POINT):
        """The irradiance a grid of baked SH9 probes gives at the caller's points (rptgpu_sample_probe_volume)
        -> a dict with one array per channel of `channels`: `value` (n, 3) float64 — the eight probes around positions[i] +
        normal_bias * normals[i], interpolated trilinearly (clamped to the grid, probes that are not valid left out and
        the weights renormalised) and convolved with the clamped cosine about normals[i], used as given; `fallback` where
        the point is not covered —, `covered` (n,) uint8 and `inside` (n,) uint8, 1 where the point lies within the grid.
        No ray is traced: the handle supplies the device.  volume: a probes.ProbeVolume.  numpy arrays go through host
        memory; torch tensors on the handle's device — points and the volume's arrays alike — are read where they lie
        (rptgpu_sample_probe_volume_device) and the results are new tensors there."""
        return self._volume_call("rptgpu_sample_probe_volume", "sample_probe_volume", positions, normals, self._POINTS, volume,
                                 normal_bias, fallback, channels, 0)

    def lookup_probe_volume(self, origins, dirs, volume, *, normal_bias=0.0, fallback=(0.0, 0.0, 0.0),
                            channels=_abi.RPT_VOLUME_ALL, flags=0):
        """The same at the first hit of each of the caller's rays (rptgpu_lookup_probe_volume) -> a dict: `t`,
        `object`, `position` — first_hits' —, `normal` — first_hits' faced to the ray —, and sample_probe_volume's `value`,
        `covered`, `inside` at that position and normal.  A miss is not covered: `value` is `fallback`, `position` and
        `normal` are zero.  origins, dirs: (n, 3) float64, used as given; numpy or torch as for sample_probe_volume."""
        return self._volume_call("rptgpu_lookup_probe_volume", "lookup_probe_volume", origins, dirs, self._RAYS, volume,
                                 normal_bias, fallback, channels, flags)

    def render_views_probe_lit(self, views, width, height, bindings, volume, *, samples=1, seed, seed_stride=0,
                               sample_index_base=0, exposure_value=0.0, filter="bilinear", normal_bias=0.0,
                               unbound_irradiance=(0.0, 0.0, 0.0), flags=0, out=None):
        """render_views_lightmapped with one change (rptgpu_render_views_probe_lit): the irradiance of a hit is
        the bound lightmap's where that covers it, else lookup_probe_volume's `value` cut at zero where `volume` covers it,
        else `unbound_irradiance`.  So what moves on a live handle, and has no chart that stays true, is lit by the probes.
        bindings may be empty.  numpy arrays — the frames then come through host memory — or torch tensors on the
        handle's device, bindings and volume alike, which give a new tensor there (out="torch" is not needed: the volume
        tells)."""
        if not _abi.probe_volume_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_render_views_probe_lit")
        who = "render_views_probe_lit"
        if filter not in self._FILTERS:
            raise ValueError('%s: filter must be "nearest" or "bilinear", not %r' % (who, filter))
        if out not in (None, "torch"):
            raise ValueError('%s: out must be None or "torch"' % who)
        n, arr, _, qv = self._view_query(who, views, width, height, 0, samples, exposure_value, seed, seed_stride, None,
                                         sample_index_base, flags)
        q = _abi.RptViewsProbeLitQuery()
        q.struct_size, q.filter, q.normal_bias = C.sizeof(q), self._FILTERS[filter], float(normal_bias)
        q.unbound_irradiance = _abi.V3(*(float(x) for x in unbound_irradiance))
        bindings = list(bindings)
        m = _marshal._Device(self.device) if out == "torch" else \
            _marshal.pick(self.device, volume.coeffs, volume.valid, *(x for b in bindings for x in (b.uvs, b.map, b.valid)))
        recs, keep = self._lower_bindings(m, bindings, who)
        rec, keep_volume = self._lower_volume(m, volume, who)
        frames = m.result(None, (n, int(height), int(width), 3), np.float64, who, "out")
        self._call("rptgpu_render_views_probe_lit", m, n, arr, C.byref(qv), len(bindings), recs, C.byref(rec), C.byref(q),
                   m.pointer(frames, C.POINTER(C.c_double)))
        del keep, keep_volume
        return frames

    @staticmethod
    def _lower_volume(m, volume, who):
        """a probes.ProbeVolume -> (an RptProbeVolume, the arrays its pointers point into)"""
        nx, ny, nz = volume.counts
        count = nx * ny * nz
        c = volume.coeffs if hasattr(volume.coeffs, "shape") else np.asarray(volume.coeffs)
        shape = tuple(int(x) for x in c.shape)
        if min(nx, ny, nz) < 0 or shape not in ((nz, ny, nx, 9, 3), (count, 9, 3)):
            raise ValueError("%s: volume.coeffs must be a (nz, ny, nx, 9, 3) or (nx * ny * nz, 9, 3) float64 array for counts %s"
                             % (who, (nx, ny, nz)))
        coeffs = m.result(c, shape, np.float64, who, "volume.coeffs")
        types = dict(_abi.RptProbeVolume._fields_)
        r = _abi.RptProbeVolume()
        r.struct_size, r.nx, r.ny, r.nz, r.reserved = C.sizeof(r), nx, ny, nz, 0
        r.origin, r.spacing = _abi.V3(*volume.origin), _abi.V3(*volume.spacing)
        # (an empty array has no address the library would take: it refuses a count of 0 before it looks)
        r.coeffs = m.field(coeffs, types["coeffs"]) if count else None
        keep = [coeffs]
        if volume.valid is not None:
            v = volume.valid if hasattr(volume.valid, "shape") else np.asarray(volume.valid)
            vshape = tuple(int(x) for x in v.shape)
            if vshape not in ((nz, ny, nx), (count,)):
                raise ValueError("%s: volume.valid must be a (nz, ny, nx) or (nx * ny * nz,) uint8 or bool array" % who)
            valid = m.flags(v, vshape, who, "volume.valid")
            r.valid = m.field(valid, types["valid"]) if count else None
            keep.append(valid)
        return r, keep

    @staticmethod
    def _lower_bindings(m, bindings, who):
        """lightmap.Binding records -> (an RptLightmapBinding array or None, the arrays its pointers point into)"""
        if not bindings:
            return None, []
        recs, keep = (_abi.RptLightmapBinding * len(bindings))(), []
        types = dict(_abi.RptLightmapBinding._fields_)
        for k, (b, r) in enumerate(zip(bindings, recs)):
            what = "bindings[%d]." % k
            uvs = m.records(b.uvs, (3, 2), who, what + "uvs")
            tex = b.map if hasattr(b.map, "shape") else np.asarray(b.map)
            if len(tex.shape) not in (2, 3) or (len(tex.shape) == 3 and int(tex.shape[2]) != 3):
                raise ValueError("%s: %smap must be an (H, W) or (H, W, 3) float64 array" % (who, what))
            height, width = int(tex.shape[0]), int(tex.shape[1])
            tex = m.result(tex, tuple(int(x) for x in tex.shape), np.float64, who, what + "map")
            r.struct_size, r.object, r.n_tris = C.sizeof(r), int(b.object), int(uvs.shape[0])
            r.width, r.height, r.components, r.reserved = width, height, 3 if len(tex.shape) == 3 else 1, 0
            # (an empty array has no address the library would take: it refuses NULL uvs, and width or height of 0)
            r.uvs = m.field(uvs, types["uvs"]) if r.n_tris else None
            r.map = m.field(tex, types["map"]) if width and height else None
            keep += [uvs, tex]
            if b.valid is not None:
                valid = m.flags(b.valid, (height, width), who, what + "valid")
                r.valid = m.field(valid, types["valid"]) if width and height else None
                keep.append(valid)
        return recs, keep

    def bake_lightmap(self, triangles, uvs, width, height, *, normals=None, samples=0, max_bounces=0, seed, offset=0.0, dilate=0,
                      channels=_abi.RPT_LIGHTMAP_IRRADIANCE | _abi.RPT_LIGHTMAP_OWNER, max_distance=float("inf"), stream_base=0,
                      sample_index_base=0, flags=0):
        """A lightmap baked on the device (rptgpu_bake_lightmap) -> a dict with one array per channel of
        `channels` (RPT_LIGHTMAP_*), each (height, width) or (height, width, 3), row 0 at v = 0: `irradiance` and `ao` —
        bake_probes' RPT_PROBE_IRRADIANCE and bake_ao's results at the texel centres the triangles' uv charts cover, from
        stream id stream_base + y * width + x, gutters filled by `dilate` rounds —, `owner` int32 (the lowest index of a
        triangle that covers the centre, -1 without one), `barycentric`, `position` (the gather point, lifted by offset *
        normal) and `normal`; +0.0 where nobody owns a texel.  triangles: world-space (n, 3, 3) float64 positions, with
        `normals` (n, 3, 3) or None (flat, Triangle.from_vertices'), or a Mesh's (n, 18) rows, positions and normals in one;
        uvs: (n, 3, 2).  numpy arrays go through host memory; torch tensors on the handle's device are read where they
        lie (rptgpu_bake_lightmap_device) and the results are new tensors there."""
        if not _abi.lightmap_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_bake_lightmap")
        who = "bake_lightmap"
        q = _abi.RptLightmapQuery()
        q.struct_size, q.channels = C.sizeof(_abi.RptLightmapQuery), int(channels)
        q.width, q.height, q.samples, q.max_bounces = int(width), int(height), int(samples), int(max_bounces)
        q.dilate, q.stream_base, q.seed, q.sample_index_base = int(dilate), int(stream_base), int(seed), int(sample_index_base)
        q.offset, q.max_distance = float(offset), float(max_distance)
        q.precision_mode, q.flags = _abi.RPT_PRECISION_F64_STRICT, int(flags)
        a = _abi.RptLightmapArrays()
        a.struct_size, a.reserved = C.sizeof(a), 0
        m = _marshal.pick(self.device, triangles, uvs, normals)
        n, pos, nrm, uv = self._lightmap_triangles(m, triangles, normals, uvs, who)
        out = m.fill(a, _marshal.layout(_marshal.LIGHTMAP_CHANNELS, q.channels, (q.height, q.width)), who)
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_bake_lightmap", m, n, m.pointer(pos, PD), m.pointer(nrm, PD), m.pointer(uv, PD), C.byref(q), C.byref(a))
        return out

    def bake_lightmap_direct(self, triangles, uvs, width, height, *, normals=None, samples, seed, offset=0.0, dilate=0,
                             stream_base=0, sample_index_base=0, flags=0):
        """The direct light of a lightmap, baked on the device (rptgpu_bake_lightmap_direct) -> (height,
        width, 3) float64: at every texel bake_lightmap owns, bake_direct's result at that texel's gather point and normal
        from stream id stream_base + y * width + x; +0.0 where nobody owns a texel; gutters filled by `dilate` rounds.
        triangles, normals, uvs, offset: bake_lightmap's.  numpy arrays go through host memory; torch tensors on the
        handle's device are read where they lie (rptgpu_bake_lightmap_direct_device) and the result is a new tensor there."""
        if not _abi.direct_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_bake_lightmap_direct")
        who = "bake_lightmap_direct"
        q = _abi.RptLightmapQuery()
        q.struct_size = C.sizeof(_abi.RptLightmapQuery)
        q.width, q.height, q.samples = int(width), int(height), int(samples)
        q.dilate, q.stream_base, q.seed, q.sample_index_base = int(dilate), int(stream_base), int(seed), int(sample_index_base)
        q.offset, q.precision_mode, q.flags = float(offset), _abi.RPT_PRECISION_F64_STRICT, int(flags)
        m = _marshal.pick(self.device, triangles, uvs, normals)
        n, pos, nrm, uv = self._lightmap_triangles(m, triangles, normals, uvs, who)
        out = m.result(None, (q.height, q.width, 3), np.float64, who, "out")
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_bake_lightmap_direct", m, n, m.pointer(pos, PD), m.pointer(nrm, PD), m.pointer(uv, PD), C.byref(q),
                   m.pointer(out, PD))
        return out

    def filter_lightmap(self, values, owner, position, normal, *, sigma_distance, sigma_plane, sigma_normal=0.1, levels=3,
                        variance=None, sigma_color=2.0, dilate=0):
        """A baked lightmap denoised on the device (rptgpu_filter_lightmap) -> `out`, shaped like `values`,
        or (out, out_variance) when `variance` is given.  values: the UNDILATED map, (height, width, 3) float64
        (bake_lightmap's `irradiance`, bake_lightmap_direct's result) or (height, width) (`ao`); owner (height, width) int32,
        position and normal (height, width, 3): the same bake's channels, the filter's guides.  `levels` a-trous passes with
        tap spacing 1, 2, 4, ... weigh a tap by exp(-e), e the sum of (1 - N_p . N_q) / sigma_normal, |N_p . (P_q - P_p)| /
        sigma_plane and |P_q - P_p|^2 / (sigma_distance * spacing)^2 — sigma_distance in world units per texel, a few of
        lightmap.texel_extent's — and, with `variance` (height, width), the variance of each texel's mean (lightmap.batch_variance),
        of the squared difference of the values over sigma_color^2 times the variances' sum.  A texel nobody owns takes
        part in nothing; `dilate` rounds of bake_lightmap's gutter fill follow.  numpy arrays go through host memory; torch
        tensors on the handle's device are read where they lie (rptgpu_filter_lightmap_device) and the results are new
        tensors there."""
        if not _abi.lightmap_filter_supported(self.lib):
            raise _abi.RptGpuError(_abi.RPTGPU_E_INVALID_ARGUMENT, "this library does not export rptgpu_filter_lightmap")
        who = "filter_lightmap"
        values, owner, position, normal = (x if hasattr(x, "shape") else np.asarray(x) for x in (values, owner, position, normal))
        m = _marshal.pick(self.device, values, owner, position, normal, variance)
        if len(owner.shape) != 2:
            raise ValueError("%s: owner must be a (height, width) int32 array" % who)
        height, width = int(owner.shape[0]), int(owner.shape[1])
        words = 3 if len(values.shape) == 3 else 1
        shape = (height, width, 3) if words == 3 else (height, width)
        f = _abi.RptLightmapFilter()
        f.struct_size, f.width, f.height, f.words = C.sizeof(f), width, height, words
        f.levels, f.dilate = int(levels), int(dilate)
        f.sigma_normal, f.sigma_plane, f.sigma_distance = float(sigma_normal), float(sigma_plane), float(sigma_distance)
        f.sigma_color = float(sigma_color)
        a = _abi.RptLightmapFilterArrays()
        a.struct_size, a.reserved = C.sizeof(a), 0
        # (m.result with an array: held to that shape, dtype and C order, and returned as it is)
        ins = {"owner": m.result(owner, (height, width), np.int32, who, "owner"),
               "position": m.result(position, (height, width, 3), np.float64, who, "position"),
               "normal": m.result(normal, (height, width, 3), np.float64, who, "normal"),
               "values": m.result(values, shape, np.float64, who, "values")}
        outs = {"out": m.room(shape, np.float64)}
        if variance is not None:
            ins["variance"] = m.result(variance, (height, width), np.float64, who, "variance")
            outs["out_variance"] = m.room((height, width), np.float64)
        types = dict(_abi.RptLightmapFilterArrays._fields_)
        for name, arr in ins.items():
            setattr(a, name, m.field(arr, types[name]))
        for name, (view, room) in outs.items():
            setattr(a, name, m.field(room, types[name]))
        self._call("rptgpu_filter_lightmap", m, C.byref(f), C.byref(a))
        out = outs["out"][0]
        return (out, outs["out_variance"][0]) if variance is not None else out

    @staticmethod
    def _lightmap_triangles(m, triangles, normals, uvs, who):
        """the lightmap calls' common half: the triangles checked -> (n, positions, normals or None, uvs)"""
        if not hasattr(triangles, "shape"):
            triangles = np.asarray(triangles)
        if len(triangles.shape) == 2:  # a Mesh's rows: v1 v2 v3 n1 n2 n3
            if normals is not None:
                raise ValueError("%s: (n, 18) triangle rows hold their normals; pass no normals beside them" % who)
            rows = m.records(triangles, (18,), who, "triangles")
            pos, nrm = rows[:, :9].reshape(-1, 3, 3), rows[:, 9:].reshape(-1, 3, 3)
        else:
            pos, nrm = triangles, normals
        pos = m.records(pos, (3, 3), who, "triangles")
        n = int(pos.shape[0])
        nrm = m.counted(m.records(nrm, (3, 3), who, "normals"), n, who, "normals", "triangles") if nrm is not None else None
        uv = m.counted(m.records(uvs, (3, 2), who, "uvs"), n, who, "uvs", "triangles")
        return n, pos, nrm, uv

    def _ray_records(self, who, origins, dirs, q, a, table):
        """first_hits' and hit_surface's common half: the rays checked, one new array per channel that q names with its
        address in `a`, then rptgpu_<who>"""
        a.struct_size, a.reserved = C.sizeof(a), 0
        m = _marshal.pick(self.device, origins, dirs)
        n, o, d = self._pair(m, origins, dirs, who, self._RAYS)  # the call's contract: (n, 3) float64 as they come
        out = m.fill(a, _marshal.layout(table, q.channels, (n,)), who)
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_" + who, m, n, m.pointer(o, PD), m.pointer(d, PD), C.byref(q), C.byref(a))
        return out

    _VERTEX_CHANNELS = _marshal.VERTEX_CHANNELS  # (scripts read it under this name)

    def trace_vertices(self, origins, dirs, max_bounces, channels=_abi.RPT_VERTEX_ALL, streams=None, samples=1, seed=0x52505447,
                       sample_index_base=0, first_draw=0, exposure_value=0.0, flags=0):
        """The vertices of the paths trace_rays runs along the caller's rays (rptgpu_trace_vertices) -> a
        PathVertices: one array per channel of `channels` (RPT_VERTEX_*), None for a channel that is not named.  With n
        rays, S = samples and B = max_bounces: `length` (n, S) uint32; per vertex (n, S, B + 1) [+ (3,)]: `t`, `normal`,
        `object` (int32), `position`, `direction`, `draw` (uint32), `radiance`, `bsdf`, `inv_pdf`, `abs_cos`; `rgb` (n, 3),
        trace_rays' result for the same arguments.  Entries behind a path's last vertex hold +0.0 (`object` -1, `draw` 0).
        origins, dirs: (n, 3) float64, used as given; streams, seed, sample_index_base, first_draw: trace_rays' stream
        contract.  numpy arrays go through host memory; torch tensors on the handle's device are read where they lie
        (rptgpu_trace_vertices_device) and the results are new tensors there (`length` and `draw` as int32: the same bits)."""
        q = _abi.RptVertexQuery()
        q.struct_size = C.sizeof(_abi.RptVertexQuery)
        q.max_bounces, q.iterations, q.first_draw = int(max_bounces), int(samples), int(first_draw)
        q.exposure_value, q.seed, q.sample_index_base = float(exposure_value), int(seed), int(sample_index_base)
        q.precision_mode, q.flags, q.channels, q.reserved = _abi.RPT_PRECISION_F64_STRICT, int(flags), int(channels), 0
        a = _abi.RptVertexArrays()
        a.struct_size, a.reserved = C.sizeof(_abi.RptVertexArrays), 0
        m = _marshal.pick(self.device, origins, dirs)
        # the call's contract: (n, 3) float64 rays as they come, but trace_rays' ids: any dtype and shape that flattens to n
        n, o, d = self._pair(m, origins, dirs, "trace_vertices", self._RAYS)
        ids = m.stream_ids(streams, n, "trace_vertices", "rays", strict=False)
        heads = {"path": (n, q.iterations), "vertex": (n, q.iterations, q.max_bounces + 1), "ray": (n,)}
        fields = [(name, heads[kind] + tail, dtype) for bit, name, kind, tail, dtype in self._VERTEX_CHANNELS if q.channels & bit]
        out = PathVertices(q.channels)
        for name, array in m.fill(a, fields, "trace_vertices").items():
            setattr(out, name, array)
        PD = C.POINTER(C.c_double)
        self._call("rptgpu_trace_vertices", m, n, m.pointer(o, PD), m.pointer(d, PD), m.pointer(ids, C.POINTER(C.c_uint32)),
                   C.byref(q), C.byref(a))
        return out

    def render_views_aov(self, views, width, height, samples=1, seed=0x52505447, seed_stride=0, sample_index_base=0,
                         channels=_abi.RPT_AOV_ALL, flags=0, out=None, seeds=None):
        """First-hit feature buffers of a batch of views (rptgpu_render_views_aov) -> a dict as render_aov's
        with the views as the leading axis: `hits` (n, H, W) uint32 always, and per channel of `channels` (RPT_AOV_*) the
        f64 sums over the hits of `samples` rays per pixel — `depth` (n, H, W), `normal` / `albedo` / `position` (n, H, W,
        3) — and `object` (n, H, W) int32.  views, seed, seed_stride, sample_index_base: render_views'; view v's rays are
        the rays render_views makes for it, so a perspective view is render_aov of its camera with seed + v * seed_stride.
        seeds: one seed per view instead, as render_views' (rptgpu_render_views_aov_seeded).
        out: None (new numpy arrays through host memory) or a dict of C-contiguous numpy arrays with exactly the keys
        above; or "torch" for new tensors on the handle's device, or a dict of contiguous torch tensors there, written
        where they lie (rptgpu_render_views_aov_device; `hits` as the 32 bits of an int32 tensor)."""
        n, arr, seed_arr, q = self._view_query("render_views_aov", views, width, height, 0, samples, 0.0, seed, seed_stride, seeds,
                                               sample_index_base, flags)
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(_abi.RptAovBuffers), int(channels)
        m, out = _marshal.pick_out(self.device, out, "render_views_aov")
        # the call's contract: new arrays are zero-initialised
        arrays = m.fill(b, _marshal.aov_layout(b.channels, (n, int(height), int(width))), "render_views_aov", out, zero=True)
        seeded = ("_seeded", seed_arr) if seed_arr is not None else ("",)
        self._call("rptgpu_render_views_aov" + seeded[0], m, n, arr, C.byref(q), *seeded[1:], C.byref(b))
        return arrays

    def render_views_denoised(self, views, width, height, max_bounces, samples, batches, seed=0x52505447, seed_stride=0,
                              seeds=None, sample_index_base=0, feature_samples=4, feature_sample_index_base=0, levels=3,
                              sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1, exposure_value=0.0,
                              flags=0, want=("denoised",), out=None):
        """A denoised frame per view in one call (rptgpu_render_views_denoised) -> a dict with one array per
        name of `want`, the views as the leading axis: `denoised` (n, H, W, 3) float64, `rgb8` (n, H, W, 3) uint8 (its
        color_bytes), `mean` (n, H, W, 3) float64 (the unfiltered mean of the batches) and `variance` (n, H, W) float64 (the
        unfiltered variance of that mean).  Per view this is DeviceBuffer.sample `batches` times — `samples` paths per pixel
        each, batch b from sample sample_index_base + b * samples —, .features with feature_samples first-hit samples from
        feature_sample_index_base, and .denoise with levels and the sigmas: a perspective view's `denoised` has that Buffer's
        bits.  views, seed, seed_stride, seeds: render_views'.  `want` must name `denoised` or `rgb8`.
        out: None (new numpy arrays through host memory) or a dict of C-contiguous numpy arrays with exactly the keys of
        `want`; or "torch" for new tensors on the handle's device, or a dict of contiguous torch tensors there, written where
        they lie (rptgpu_render_views_denoised_device)."""
        n, arr, seed_arr, q = self._view_query("render_views_denoised", views, width, height, max_bounces, samples, exposure_value,
                                               seed, seed_stride, seeds, sample_index_base, flags)
        want = (want,) if isinstance(want, str) else tuple(want)
        known = [name for name, _, _ in _marshal.DENOISED_OUTPUTS]
        if not want or len(set(want)) != len(want) or any(w not in known for w in want):
            raise ValueError("render_views_denoised: want must name each of %s at most once, and one at least" % (known,))
        if "denoised" not in want and "rgb8" not in want:
            raise ValueError("render_views_denoised: want must name `denoised` or `rgb8`")
        d = _abi.RptViewDenoise()
        d.struct_size, d.batches, d.feature_iterations = C.sizeof(_abi.RptViewDenoise), int(batches), int(feature_samples)
        d.feature_sample_index_base = int(feature_sample_index_base)
        d.filter.struct_size, d.filter.levels = C.sizeof(_abi.RptDenoise), int(levels)
        d.filter.sigma_color, d.filter.sigma_normal = float(sigma_color), float(sigma_normal)
        d.filter.sigma_depth, d.filter.sigma_albedo = float(sigma_depth), float(sigma_albedo)
        o = _abi.RptViewDenoiseOut()
        o.struct_size = C.sizeof(_abi.RptViewDenoiseOut)
        m, out = _marshal.pick_out(self.device, out, "render_views_denoised")
        head = (n, int(height), int(width))
        fields = [(name, head + tail, dtype) for name, tail, dtype in _marshal.DENOISED_OUTPUTS if name in want]
        arrays = m.fill(o, fields, "render_views_denoised", out)
        # (seeds or NULL: one symbol)
        self._call("rptgpu_render_views_denoised", m, n, arr, C.byref(q), seed_arr, C.byref(d), C.byref(o))
        return arrays

    @staticmethod
    def _lower_seeds(seeds, n, seed_stride, who):
        """seeds=None -> None; else the n seeds as a ctypes uint64 array (at least one element: it has an address)"""
        if seeds is None:
            return None
        if int(seed_stride) != 0:
            raise ValueError("%s: seeds and a non-zero seed_stride exclude each other" % who)
        if isinstance(seeds, np.ndarray) and seeds.dtype != np.uint64:
            raise ValueError("%s: a numpy array of seeds must be uint64" % who)
        values = [int(s) for s in seeds]
        if len(values) != n:
            raise ValueError("%s: %d seeds for %d views" % (who, len(values), n))
        if any(not 0 <= s < 1 << 64 for s in values):
            raise ValueError("%s: a seed must fit 64 bits unsigned" % who)
        arr = (C.c_uint64 * max(n, 1))()
        arr[:n] = values
        return arr

    @staticmethod
    def _lower_views(views, who):
        arr = (_abi.RptView * max(len(views), 1))()
        for i, v in enumerate(views):
            if isinstance(v, _abi.RptView):
                arr[i] = v
            elif hasattr(v, "projection"):
                arr[i] = v.lower()
            elif hasattr(v, "lower"):
                arr[i].camera, arr[i].projection = v.lower(), _abi.RPT_VIEW_PERSPECTIVE
            else:
                raise TypeError("%s: view %d is a %s, not a View, a Camera or an RptView" % (who, i, type(v).__name__))
        return arr

    def render_aov(self, camera, params, channels=_abi.RPT_AOV_ALL):
        """First-hit feature buffers (rptgpu_render_aov) -> a dict of numpy arrays: `hits` (H, W) uint32
        always, and per channel of `channels` (RPT_AOV_*) the f64 SUMS over the hits of params.iterations camera rays per
        pixel — `depth` (H, W), `normal` / `albedo` / `position` (H, W, 3) — and `object` (H, W) int32, the object the
        call's first sample hit (-1: none).  A mean is sum / hits."""
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(_abi.RptAovBuffers), int(channels)
        arrays = _marshal.HOST.fill(b, _marshal.aov_layout(b.channels, (params.height, params.width)), "render_aov", zero=True)
        cam = _lower_camera(camera)
        _abi.check(self.lib.rptgpu_render_aov(self.handle, C.byref(cam), C.byref(params), C.byref(b)), self.handle)
        return arrays

    def eval_math(self, fn, x, y=None):
        """include/rpt_math.h evaluated on the device (diagnostics)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        yy = np.ascontiguousarray(y, dtype=np.float64) if y is not None else None
        out = np.empty_like(x)
        PD = C.POINTER(C.c_double)
        code = self.lib.rptgpu_eval_math(self.handle, int(fn), x.size, x.ctypes.data_as(PD),
                                         yy.ctypes.data_as(PD) if yy is not None else None, out.ctypes.data_as(PD))
        _abi.check(code, self.handle)
        return out

    def stats(self):
        s = _abi.RptStats()
        _abi.check(self.lib.rptgpu_get_stats(self.handle, C.byref(s)), self.handle)
        return s

    def reset_stats(self):
        _abi.check(self.lib.rptgpu_reset_stats(self.handle), self.handle)


def kdtree_build(boxes, lib=None, prefix="rptgpu", device=None):
    """KdTree::new over (n, 6) boxes through the C ABI -> dict of numpy arrays.  device: build on that HIP device
    (rptgpu_kdtree_build_device) instead of the host."""
    lib = lib or _abi.load_library()
    b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    t = _abi.RptKdTree()
    free = getattr(lib, prefix + "_kdtree_free")
    if device is None:
        code = getattr(lib, prefix + "_kdtree_build")(b.ctypes.data_as(C.POINTER(C.c_double)), len(b), C.byref(t))
    else:
        code = lib.rptgpu_kdtree_build_device(b.ctypes.data_as(C.POINTER(C.c_double)), len(b), int(device), C.byref(t))
    if code != 0:
        detail = lib.rptgpu_last_error_detail(None) if prefix == "rptgpu" else b""
        raise _abi.RptGpuError(code, "kdtree_build: " + (detail.decode() if detail else ""))
    n, r = t.num_nodes, t.num_refs
    out = {
        "split": np.ctypeslib.as_array(t.split, (n,)).copy(),
        "info": np.ctypeslib.as_array(t.info, (n,)).copy(),
        "a": np.ctypeslib.as_array(t.a, (n,)).copy(),
        "b": np.ctypeslib.as_array(t.b, (n,)).copy(),
        "refs": np.ctypeslib.as_array(t.refs, (max(r, 1),)).copy()[:r],
        "max_depth": t.max_depth,
        "regular": t.regular,
    }
    free(C.byref(t))
    return out


class DeviceBuffer:
    """`Buffer` (reference src/buffer.rs) kept on the GPU: `rptgpu_buffer_*` of include/rpt_gpu.h.
    Same results as the host `rpt_amd.Buffer`, without moving any batch to the host."""

    def __init__(self, gpu_scene, width, height, filter=None):
        self.gpu = gpu_scene
        self.width, self.height = int(width), int(height)
        radius = filter.radius if filter is not None else 0
        h = C.c_void_p()
        _abi.check(gpu_scene.lib.rptgpu_buffer_create(gpu_scene.handle, self.width, self.height, int(radius), C.byref(h)),
                   gpu_scene.handle)
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.gpu.lib.rptgpu_buffer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample(self, camera, params):
        """Renderer::sample + Buffer::add_samples on the device."""
        cam = _lower_camera(camera)
        _abi.check(self.gpu.lib.rptgpu_buffer_sample(self.handle, C.byref(cam), C.byref(params)), self.gpu.handle)

    def image(self):
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        _abi.check(self.gpu.lib.rptgpu_buffer_image(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint8))), self.gpu.handle)
        return out

    def variance(self):
        v = C.c_double(0.0)
        _abi.check(self.gpu.lib.rptgpu_buffer_variance(self.handle, C.byref(v)), self.gpu.handle)
        return v.value

    def num_batches(self):
        n = C.c_uint32(0)
        _abi.check(self.gpu.lib.rptgpu_buffer_num_batches(self.handle, C.byref(n)), self.gpu.handle)
        return n.value

    # ---- adaptive sampling (rptgpu_buffer_sample_adaptive)
    def sample_adaptive(self, camera, params, min_batches=4, abs_tol=0.0, rel_tol=0.01):
        """One batch for the pixels still active, then the stopping rule -> the number of pixels active afterwards.  Once
        a pixel has retired, sample() is refused."""
        cam = _lower_camera(camera)
        a = _abi.RptAdaptive(C.sizeof(_abi.RptAdaptive), int(min_batches), float(abs_tol), float(rel_tol))
        n = C.c_uint32(0)
        _abi.check(self.gpu.lib.rptgpu_buffer_sample_adaptive(self.handle, C.byref(cam), C.byref(params), C.byref(a),
                                                              C.byref(n)), self.gpu.handle)
        return n.value

    def sample_counts(self):
        """(H, W) uint32: the batches each pixel holds."""
        out = np.empty((self.height, self.width), dtype=np.uint32)
        _abi.check(self.gpu.lib.rptgpu_buffer_sample_counts(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint32))),
                   self.gpu.handle)
        return out

    def totals(self):
        """(H, W, 3) float64: the sum of each pixel's batch values (the linear mean is totals / sample_counts)."""
        out = np.empty((self.height, self.width, 3), dtype=np.float64)
        _abi.check(self.gpu.lib.rptgpu_buffer_totals(self.handle, out.ctypes.data_as(C.POINTER(C.c_double))),
                   self.gpu.handle)
        return out

    # ---- feature-guided denoising (rptgpu_buffer_features / _denoise)
    def features(self, camera, params):
        """The first-hit features of (camera, params) — GpuScene.render_aov's depth, normal, albedo and position sums and
        `hits` — computed into device arrays the buffer keeps (nothing comes to the host); they guide denoise().  A later
        call replaces them."""
        cam = _lower_camera(camera)
        _abi.check(self.gpu.lib.rptgpu_buffer_features(self.handle, C.byref(cam), C.byref(params)), self.gpu.handle)

    def feature_sums(self):
        """The held features read back: GpuScene.render_aov's dict without `object`."""
        b = _abi.RptAovBuffers()
        b.struct_size, b.channels = C.sizeof(_abi.RptAovBuffers), _abi.RPT_AOV_ALL & ~_abi.RPT_AOV_OBJECT
        arrays = _marshal.HOST.fill(b, _marshal.aov_layout(b.channels, (self.height, self.width)), "feature_sums", zero=True)
        _abi.check(self.gpu.lib.rptgpu_buffer_feature_sums(self.handle, C.byref(b)), self.gpu.handle)
        return arrays

    def _denoise(self, want_linear, want_bytes, levels, sigma_color, sigma_normal, sigma_depth, sigma_albedo):
        d = _abi.RptDenoise(C.sizeof(_abi.RptDenoise), int(levels), float(sigma_color), float(sigma_normal),
                            float(sigma_depth), float(sigma_albedo))
        lin = np.empty((self.height, self.width, 3), dtype=np.float64) if want_linear else None
        rgb = np.empty((self.height, self.width, 3), dtype=np.uint8) if want_bytes else None
        _abi.check(self.gpu.lib.rptgpu_buffer_denoise(
            self.handle, C.byref(d), lin.ctypes.data_as(C.POINTER(C.c_double)) if want_linear else None,
            rgb.ctypes.data_as(C.POINTER(C.c_uint8)) if want_bytes else None), self.gpu.handle)
        return lin, rgb

    def denoise(self, levels=3, sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1):
        """The buffer's linear mean through the edge-avoiding a-trous filter of include/rpt_gpu.h, guided by the held
        features and the per-pixel variance -> (H, W, 3) float64.  The buffer itself is not changed."""
        return self._denoise(True, False, levels, sigma_color, sigma_normal, sigma_depth, sigma_albedo)[0]

    def denoised_image(self, levels=3, sigma_color=2.0, sigma_normal=0.1, sigma_depth=0.01, sigma_albedo=0.1):
        """color_bytes of denoise(...) -> (H, W, 3) uint8."""
        return self._denoise(False, True, levels, sigma_color, sigma_normal, sigma_depth, sigma_albedo)[1]
