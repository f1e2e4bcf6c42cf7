"""What a caller of GpuScene.bake_lightmap needs beside it (include/rpt_gpu_lightmap.h): the texture
coordinates of an OBJ's triangles, in the order load_obj makes the triangles, a bake turned into bytes to look at, and what
GpuScene.filter_lightmap wants beside a bake: the world size of a texel and a variance from several bakes.
numpy only."""
import numpy as np

from .color import color_bytes
from .io import _at, _lines, _open, _parse_index


def load_obj_texcoords(file):
    """-> (n_tris, 3, 2) float64: the `vt` of every triangle load_obj(file) makes, in its order — faces fan-triangulated
    (io.rs:181-198: corners 0, i, i + 1), indices by _parse_index (1-based, or negative from the end of what was read so
    far) and looked up with _at (out of range raises IndexError, as the reference panics).  ValueError if any face corner
    has no `vt` index: such a mesh has no chart to bake into.  A `vt` line's third coordinate is not read."""
    f, own = _open(file, "r")
    try:
        n_vertices, texcoords, out = 0, [], []
        for tokens in _lines(f):
            if tokens[0] == "v":
                n_vertices += 1
            elif tokens[0] == "vt":
                try:
                    texcoords.append((float(tokens[1]), float(tokens[2])))
                except (ValueError, IndexError):
                    raise ValueError("Failed to parse texture coordinate in .OBJ")
            elif tokens[0] == "f":
                vti = []
                for vertex in tokens[1:]:
                    args = (vertex.split("/") + ["", "", ""])[:3]
                    if _parse_index(args[0], n_vertices) is None:
                        raise ValueError("Invalid vertex index")
                    t = _parse_index(args[1], len(texcoords))
                    if t is None:
                        raise ValueError("load_obj_texcoords: face corner %r has no vt index" % vertex)
                    vti.append(t)
                for i in range(1, len(vti) - 1):
                    out.append((_at(texcoords, vti[0]), _at(texcoords, vti[i]), _at(texcoords, vti[i + 1])))
        return np.array(out, dtype=np.float64).reshape(-1, 3, 2)
    finally:
        if own:
            f.close()


class Binding:
    """One baked map tied to one object of a scene, for GpuScene.lookup_lightmap (include/rpt_gpu_lightmap_lookup.h,
    DESIGN.md §25): `object`, the index of a top-level object whose shape is a mesh (plain or Transformed); `uvs`
    (n_tris, 3, 2) float64 in the mesh's own triangle order; `map` (H, W) or (H, W, 3) float64, row 0 at v = 0 as
    bake_lightmap writes it; `valid` (H, W) uint8 or bool, non-zero where the texel holds a value (a bake's owner >= 0), or
    None: every texel does.  numpy arrays or torch tensors on the handle's device, all of one kind; they are checked by
    the call."""

    def __init__(self, object, uvs, map, valid=None):
        self.object, self.uvs, self.map, self.valid = int(object), uvs, map, valid


def texel_extent(position, owner):
    """The median world distance between horizontally adjacent owned texels of a bake: `position` (H, W, 3) and `owner`
    (H, W) of bake_lightmap.  GpuScene.filter_lightmap's sigma_distance is a few of these.  ValueError when no two owned
    texels are neighbours in a row."""
    position = np.asarray(position, dtype=np.float64)
    owned = np.asarray(owner) >= 0
    pair = owned[:, 1:] & owned[:, :-1]
    if not pair.any():
        raise ValueError("texel_extent: no two owned texels are neighbours in a row")
    d = position[:, 1:] - position[:, :-1]
    return float(np.median(np.sqrt((d * d).sum(axis=-1))[pair]))


def batch_variance(bakes):
    """-> (mean, variance): from B >= 2 bakes of one map, each (H, W) or (H, W, 3) — the same call with
    sample_index_base advanced by `samples` from bake to bake, so that their samples are independent —, the mean over the
    bakes per texel and the variance of THAT MEAN per texel, summed over the components: Welford's recurrence (the device
    Buffer's), M2 / (B - 1) / B.  What GpuScene.filter_lightmap takes as `values` and `variance`."""
    bakes = [np.asarray(b, dtype=np.float64) for b in bakes]
    if len(bakes) < 2:
        raise ValueError("batch_variance: a variance takes two bakes at least")
    flat = bakes[0].ndim == 2
    mean = np.zeros(bakes[0].shape if not flat else bakes[0].shape + (1,))
    m2 = np.zeros(mean.shape[:2])
    with np.errstate(all="ignore"):
        for k, b in enumerate(bakes):
            x = b.reshape(mean.shape)
            d = x - mean
            mean = mean + d / np.float64(k + 1)
            m2 = m2 + (d * (x - mean)).sum(axis=-1)
        n = np.float64(len(bakes))
        variance = (m2 / (n - 1.0)) / n
    return (mean[..., 0] if flat else mean), variance


def to_rgb8(irradiance, albedo=(1.0, 1.0, 1.0), exposure=0.0):
    """(H, W, 3) uint8 to look at a bake: the radiance a diffuse surface of `albedo` sends out under `irradiance`,
    albedo / pi * irradiance * 2^exposure, through color_bytes."""
    radiance = np.asarray(irradiance, dtype=np.float64) * (np.asarray(albedo, dtype=np.float64) / np.pi * 2.0 ** float(exposure))
    return color_bytes(radiance)
