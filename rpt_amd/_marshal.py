"""What device.py's array calls need from the caller's arrays, once: two backends with one interface — HOST for numpy
arrays, which go to the library's host symbols as ctypes pointers, and a device backend for torch tensors on the handle's
device, which go to the `_device` symbols as addresses, behind the null-stream rule — and the tables of the channels the
calls return.  Host-only Python; torch is imported only where a tensor came in."""
import ctypes as C

import numpy as np

from . import _abi

# ---- the channels of the calls that return several arrays: (bit, name, shape behind the leading axes, dtype)
HIT_CHANNELS = ((_abi.RPT_HIT_T, "t", (), np.float64), (_abi.RPT_HIT_NORMAL, "normal", (3,), np.float64),
                (_abi.RPT_HIT_OBJECT, "object", (), np.int32), (_abi.RPT_HIT_POSITION, "position", (3,), np.float64),
                (_abi.RPT_HIT_ALBEDO, "albedo", (3,), np.float64))
SURFACE_CHANNELS = ((_abi.RPT_SURFACE_T, "t", (), np.float64), (_abi.RPT_SURFACE_OBJECT, "object", (), np.int32),
                    (_abi.RPT_SURFACE_CHILD, "child", (), np.int32), (_abi.RPT_SURFACE_PRIMITIVE, "primitive", (), np.int32),
                    (_abi.RPT_SURFACE_BARYCENTRIC, "barycentric", (3,), np.float64))
LIGHTMAP_CHANNELS = ((_abi.RPT_LIGHTMAP_IRRADIANCE, "irradiance", (3,), np.float64), (_abi.RPT_LIGHTMAP_AO, "ao", (), np.float64),
                     (_abi.RPT_LIGHTMAP_OWNER, "owner", (), np.int32), (_abi.RPT_LIGHTMAP_BARYCENTRIC, "barycentric", (3,), np.float64),
                     (_abi.RPT_LIGHTMAP_POSITION, "position", (3,), np.float64), (_abi.RPT_LIGHTMAP_NORMAL, "normal", (3,), np.float64))
LOOKUP_CHANNELS = ((_abi.RPT_LOOKUP_T, "t", (), np.float64), (_abi.RPT_LOOKUP_OBJECT, "object", (), np.int32),
                   (_abi.RPT_LOOKUP_BINDING, "binding", (), np.int32), (_abi.RPT_LOOKUP_COVERED, "covered", (), np.uint8),
                   (_abi.RPT_LOOKUP_UV, "uv", (2,), np.float64), (_abi.RPT_LOOKUP_VALUE, "value", (3,), np.float64))
VOLUME_CHANNELS = ((_abi.RPT_VOLUME_T, "t", (), np.float64), (_abi.RPT_VOLUME_OBJECT, "object", (), np.int32),
                   (_abi.RPT_VOLUME_POSITION, "position", (3,), np.float64), (_abi.RPT_VOLUME_NORMAL, "normal", (3,), np.float64),
                   (_abi.RPT_VOLUME_VALUE, "value", (3,), np.float64), (_abi.RPT_VOLUME_COVERED, "covered", (), np.uint8),
                   (_abi.RPT_VOLUME_INSIDE, "inside", (), np.uint8))
# rptgpu_trace_vertices': (bit, name, "path" | "vertex" | "ray", shape behind it, dtype)
VERTEX_CHANNELS = ((_abi.RPT_VERTEX_LENGTH, "length", "path", (), np.uint32), (_abi.RPT_VERTEX_T, "t", "vertex", (), np.float64),
                   (_abi.RPT_VERTEX_NORMAL, "normal", "vertex", (3,), np.float64),
                   (_abi.RPT_VERTEX_OBJECT, "object", "vertex", (), np.int32),
                   (_abi.RPT_VERTEX_POSITION, "position", "vertex", (3,), np.float64),
                   (_abi.RPT_VERTEX_DIRECTION, "direction", "vertex", (3,), np.float64),
                   (_abi.RPT_VERTEX_DRAW, "draw", "vertex", (), np.uint32),
                   (_abi.RPT_VERTEX_RADIANCE, "radiance", "vertex", (3,), np.float64),
                   (_abi.RPT_VERTEX_BSDF, "bsdf", "vertex", (3,), np.float64),
                   (_abi.RPT_VERTEX_INV_PDF, "inv_pdf", "vertex", (), np.float64),
                   (_abi.RPT_VERTEX_ABS_COS, "abs_cos", "vertex", (), np.float64),
                   (_abi.RPT_VERTEX_RGB, "rgb", "ray", (3,), np.float64))
AOV_CHANNELS = ((_abi.RPT_AOV_DEPTH, "depth", (), np.float64), (_abi.RPT_AOV_NORMAL, "normal", (3,), np.float64),
                (_abi.RPT_AOV_ALBEDO, "albedo", (3,), np.float64), (_abi.RPT_AOV_POSITION, "position", (3,), np.float64),
                (_abi.RPT_AOV_OBJECT, "object", (), np.int32))
# rptgpu_render_views_denoised's outputs, by name: (name, shape behind (n, H, W), dtype)
DENOISED_OUTPUTS = (("denoised", (3,), np.float64), ("rgb8", (3,), np.uint8), ("mean", (3,), np.float64),
                    ("variance", (), np.float64))


def layout(table, channels, head):
    """[(name, shape, dtype)] of the channels of `table` that `channels` names, `head` the leading axes"""
    return [(name, head + tail, dtype) for bit, name, tail, dtype in table if channels & bit]


def aov_layout(channels, head):
    """RptAovBuffers' arrays: `hits` always, then the named channels"""
    return [("hits", head, np.uint32)] + layout(AOV_CHANNELS, channels, head)


class _Backend:
    """what the two backends share: the steps that are written against the others"""

    def counted(self, a, n, who, what, noun):
        """`a` with its leading axis held to n"""
        if int(a.shape[0]) != n:
            raise ValueError("%s: %d %s for %d %s" % (who, int(a.shape[0]), what, n, noun))
        return a

    def room(self, shape, dtype, zero=False):
        """-> (view, owner): a new array of `shape` and the allocation behind it, which has one element at least — an
        empty array has no address, and a named output's pointer must not be NULL"""
        count = int(np.prod(shape))
        owner = self.new(max(count, 1), dtype, zero)
        return owner[:count].reshape(shape), owner

    def fill(self, struct, fields, who, out=None, zero=False):
        """The pointers of an output struct (RptHitArrays, RptSurfaceArrays, RptLightmapArrays, RptVertexArrays,
        RptAovBuffers, RptViewDenoiseOut) from `fields`, [(name, shape, dtype)] -> {name: array}: new arrays with room behind them, or
        the caller's `out`, a dict with exactly these names, checked and written where they lie."""
        if out is None:
            rooms = {name: self.room(shape, dtype, zero) for name, shape, dtype in fields}
            arrays, owners = {name: r[0] for name, r in rooms.items()}, {name: r[1] for name, r in rooms.items()}
        else:
            arrays = owners = dict(out)
            if set(arrays) != {name for name, _, _ in fields}:
                raise ValueError("%s: out must have exactly the keys %s" % (who, sorted(name for name, _, _ in fields)))
            for name, shape, dtype in fields:
                self.result(arrays[name], shape, dtype, who, "out[%r]" % name)
        types = dict(type(struct)._fields_)
        for name, owner in owners.items():
            setattr(struct, name, self.field(owner, types[name]))
        return arrays


class _Host(_Backend):
    """numpy arrays in host memory; the library's host symbols"""
    suffix = ""

    def vectors(self, a, who, what, coerce=False):
        if coerce:
            return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)
        a = np.asarray(a)
        if a.dtype != np.float64 or a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("%s: %s must be an (n, 3) float64 array" % (who, what))
        return np.ascontiguousarray(a)

    def stream_ids(self, a, n, who, noun, strict):
        if a is None:
            return None
        if strict:
            a = np.asarray(a)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError("%s: streams must be an (n,) integer array" % who)
        return self.counted(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1), n, who, "stream ids", noun)

    def scalars(self, a, n, who, what):
        if a is None:
            return None
        a = np.asarray(a)
        if a.dtype != np.float64 or a.shape != (n,):
            raise ValueError("%s: %s must be an (n,) float64 array" % (who, what))
        return np.ascontiguousarray(a)

    def rows(self, a, width, who, what):
        """set_mesh's and set_group's (n, width) float64 records"""
        a = np.asarray(a)
        if a.dtype != np.float64:
            raise TypeError("%s: %s must be float64, not %s" % (who, what, a.dtype))
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError("%s: %s must have shape (n, %d), not %s" % (who, what, width, tuple(a.shape)))
        return np.ascontiguousarray(a)

    def records(self, a, tail, who, what):
        """bake_lightmap's (n,) + tail float64 records -> a contiguous array of that shape"""
        a = np.asarray(a)
        if a.dtype != np.float64 or a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
            raise ValueError("%s: %s must be an (n, %s) float64 array" % (who, what, ", ".join(str(t) for t in tail)))
        return np.ascontiguousarray(a)

    def flags(self, a, shape, who, what):
        """a lightmap binding's valid map: `shape` bytes or bools -> contiguous uint8"""
        a = np.asarray(a)
        if a.dtype not in (np.uint8, np.bool_) or a.shape != tuple(shape):
            raise ValueError("%s: %s must be a %s uint8 or bool array" % (who, what, tuple(shape)))
        return np.ascontiguousarray(a).view(np.uint8)

    def new(self, count, dtype, zero):
        return (np.zeros if zero else np.empty)(count, dtype=dtype)

    def result(self, a, shape, dtype, who, what):
        dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
        if a is None:
            return np.empty(shape, dtype=dtypes[0])
        if not (isinstance(a, np.ndarray) and a.dtype in dtypes and a.shape == tuple(shape) and a.flags.c_contiguous):
            raise ValueError("%s: %s must be a C-contiguous %s %s array"
                             % (who, what, tuple(shape), " or ".join(np.dtype(d).name for d in dtypes)))
        return a

    def pointer(self, a, ctype):
        return a.ctypes.data_as(ctype) if a is not None else None

    field = pointer

    def stream_args(self):
        return ()


HOST = _Host()


class _Device(_Backend):
    """torch tensors on the handle's device; the library's `_device` symbols, which take addresses and a stream"""
    suffix = "_device"

    def __init__(self, device):
        import torch
        self.torch, self.index, self.dev = torch, int(device), torch.device("cuda", int(device))
        # (uint32 arrays are the 32 bits of an int32 tensor)
        self.dtypes = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8,
                       np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32}

    def here(self, a, who, what):
        if not isinstance(a, self.torch.Tensor) or a.device != self.dev:
            raise ValueError("%s: %s must be a torch tensor on %s, like the other arrays" % (who, what, self.dev))
        return a

    def vectors(self, a, who, what, coerce=False):
        self.here(a, who, what)
        if coerce:
            return a.to(self.torch.float64).reshape(-1, 3).contiguous()  # (no copy when it already is all that)
        if a.dtype != self.torch.float64 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError("%s: %s must be an (n, 3) float64 tensor" % (who, what))
        return a.contiguous()  # (no copy when it already is)

    def stream_ids(self, a, n, who, noun, strict):
        if a is None:
            return None
        self.here(a, who, "streams")
        if strict and (a.dim() != 1 or a.dtype.is_floating_point):
            raise ValueError("%s: streams must be an (n,) integer tensor" % who)
        a = a.reshape(-1)
        if a.dtype not in (self.torch.int32, getattr(self.torch, "uint32", self.torch.int32)):
            a = a.to(self.torch.int64).to(self.torch.int32)  # the low 32 bits
        return self.counted(a.contiguous(), n, who, "stream ids", noun)

    def scalars(self, a, n, who, what):
        if a is None:
            return None
        self.here(a, who, what)
        if a.dtype != self.torch.float64 or tuple(a.shape) != (n,):
            raise ValueError("%s: %s must be an (n,) float64 tensor" % (who, what))
        return a.contiguous()

    def rows(self, a, width, who, what):
        """set_mesh's and set_group's (n, width) float64 records: read where they lie, so contiguous as they come"""
        if a.dtype != self.torch.float64:
            raise TypeError("%s: %s must be float64, not %s" % (who, what, a.dtype))
        if a.dim() != 2 or a.shape[1] != width:
            raise ValueError("%s: %s must have shape (n, %d), not %s" % (who, what, width, tuple(a.shape)))
        if not a.is_cuda or a.device.index != self.index:
            raise ValueError("%s: the tensor is on %s, the handle on device %d (pass a numpy array for host data)"
                             % (who, a.device, self.index))
        if not a.is_contiguous():
            raise ValueError("%s: the tensor must be contiguous" % who)
        return a

    def records(self, a, tail, who, what):
        """bake_lightmap's (n,) + tail float64 records -> a contiguous tensor of that shape (no copy when it already is)"""
        self.here(a, who, what)
        if a.dtype != self.torch.float64 or a.dim() != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
            raise ValueError("%s: %s must be an (n, %s) float64 tensor" % (who, what, ", ".join(str(t) for t in tail)))
        return a.contiguous()

    def flags(self, a, shape, who, what):
        """a lightmap binding's valid map: `shape` bytes or bools -> a contiguous uint8 tensor"""
        self.here(a, who, what)
        if a.dtype not in (self.torch.uint8, self.torch.bool) or tuple(a.shape) != tuple(shape):
            raise ValueError("%s: %s must be a %s uint8 or bool tensor" % (who, what, tuple(shape)))
        return a.to(self.torch.uint8).contiguous()

    def new(self, count, dtype, zero):
        return (self.torch.zeros if zero else self.torch.empty)(count, dtype=self.dtypes[np.dtype(dtype)], device=self.dev)

    def result(self, a, shape, dtype, who, what):
        dtypes = [self.dtypes[np.dtype(d)] for d in (dtype if isinstance(dtype, tuple) else (dtype,))]
        if a is None:
            return self.torch.empty(tuple(shape), dtype=dtypes[0], device=self.dev)
        if not (isinstance(a, self.torch.Tensor) and a.device == self.dev and a.dtype in dtypes and tuple(a.shape) == tuple(shape)
                and a.is_contiguous()):
            raise ValueError("%s: %s must be a contiguous %s %s tensor on %s"
                             % (who, what, tuple(shape), " or ".join(str(d) for d in dtypes), self.dev))
        return a

    def pointer(self, a, ctype):
        return C.c_void_p(a.data_ptr()) if a is not None else None

    def field(self, a, ctype):
        return C.cast(C.c_void_p(a.data_ptr()), ctype)

    def stream_args(self):
        """THE NULL-STREAM RULE.  The tensors' producer — and any conversion made here — ran on torch's current stream;
        the handle's own stream is non-blocking, so nothing orders the two by itself.  A stream with a handle is handed
        to the library, which waits for it; torch's default stream is the null stream, whose handle 0 is the ABI's "no
        stream": that one is waited for here."""
        current = self.torch.cuda.current_stream(self.dev)
        stream = current.cuda_stream
        if not stream:
            current.synchronize()
        return (C.c_void_p(stream or 0),)


def pick(device, *arrays):
    """the device backend of the handle on `device` when any of `arrays` is a torch tensor (it then refuses whatever is
    not a tensor there), else HOST"""
    return _Device(device) if any(hasattr(a, "data_ptr") for a in arrays) else HOST


def pick_out(device, out, who):
    """(backend, out) of the calls that return a dict: None or a dict of numpy arrays -> HOST; "torch" -> new tensors on
    the handle's device; anything else is taken for a dict of tensors there"""
    if out is None or (isinstance(out, dict) and all(isinstance(v, np.ndarray) for v in out.values())):
        return HOST, out
    if isinstance(out, str):
        if out != "torch":
            raise ValueError('%s: out must be None, "torch" or a dict of arrays or tensors' % who)
        return _Device(device), None
    return _Device(device), out
