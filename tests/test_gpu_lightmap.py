"""rptgpu_bake_lightmap on the GPU, held to include/rpt_gpu_lightmap.h to the bit.

The raster — owners, barycentrics, gather points, normals — against tests/lightmap_model.py, the header restated in numpy
(itself held to closed forms in tests/test_lightmap_host.py); the gathers against the calls they are defined by, bake_probes
and bake_ao at the call's own POSITION and NORMAL with the texels' stream ids; the independence the header promises — of
pieces, stream_base, route, host or device arrays, the channels named, a live update —; the dilation against the model applied
to the call's own undilated output.  Every comparison is on the bits (lightmap_model.same)."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

import rpt_amd
from rpt_amd import GpuScene, _abi

import lightmap_model as M
import small_scenes
import surface_model

pytestmark = pytest.mark.gpu

IRR, AO, OWNER = _abi.RPT_LIGHTMAP_IRRADIANCE, _abi.RPT_LIGHTMAP_AO, _abi.RPT_LIGHTMAP_OWNER
BARY, POS, NRM = _abi.RPT_LIGHTMAP_BARYCENTRIC, _abi.RPT_LIGHTMAP_POSITION, _abi.RPT_LIGHTMAP_NORMAL
RAW = OWNER | BARY | POS | NRM
ALL = _abi.RPT_LIGHTMAP_ALL
RAW_NAMES = ("owner", "barycentric", "position", "normal")
SCENES = ["cornell", "wine_glass"]   # the flat route and the per-tree route
SAMPLES, BOUNCES, SEED = 8, 3, 0x4C4D
# where the synthetic triangles stand: inside the box of each scene (tests/test_gpu_probes.py BOXES)
BOXES = {"cornell": ((20.0, 20.0, 20.0), (536.0, 528.0, 540.0)), "wine_glass": ((-2.0, 0.1, -2.0), (2.0, 4.0, 2.0))}


@functools.lru_cache(maxsize=None)
def gpu(name):
    return GpuScene(small_scenes.small(name)[0], 0)


def differing(got, want, names=None):
    names = sorted(want) if names is None else names
    return [k for k in names if k not in got or not M.same(np.asarray(got[k]), np.asarray(want[k]))]


# ---- the charts.  uv triangles by name; positions and normals are drawn per case inside the scene's box
def quad(lo=1.0 / 16.0, hi=15.0 / 16.0):
    return [[[lo, lo], [hi, lo], [hi, hi]], [[lo, lo], [hi, hi], [lo, hi]]]


NAN = float("nan")
ZOO = [[[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]],            # 0: zero area
       [[0.1, 0.1], [NAN, 0.2], [0.3, 0.9]],            # 1: a NaN uv
       [[1.5, 1.5], [2.5, 1.5], [1.5, 2.5]],            # 2: wholly outside the map
       [[0.05, 0.05], [0.05, 0.45], [0.45, 0.05]],      # 3: a mirrored chart (area < 0)
       [[0.2, 0.2], [0.6, 0.2], [0.2, 0.6]],            # 4: overlaps 3
       [[0.7, 0.3], [1.4, 0.3], [0.7, 0.9]],            # 5: hangs over the map's right edge
       [[-50.0, -40.0], [60.0, -45.0], [0.0, 70.0]]]    # 6: much larger than the map: everything the others leave
CHARTS = {"quad": quad(), "zoo": ZOO, "zoo_reversed": ZOO[::-1]}
# (the rasteriser strides a triangle's box of texels with one wavefront up to 4096 texels and hands a larger one to a second
# launch: the zoo's last triangle has the whole map for its box — 64 x 64 is the last size of the first path, 65 x 64 the
# first of the second, 80 x 70 well inside it; the quad's two boxes of 68 x 68 on a 72 x 72 map go the second way together)
RASTER_CASES = [("quad", 16, 16), ("quad", 13, 7), ("zoo", 16, 16), ("zoo", 13, 7), ("zoo", 1, 1), ("quad", 1, 1),
                ("zoo_reversed", 16, 16), ("zoo_reversed", 13, 7), ("zoo", 64, 64), ("zoo", 65, 64), ("zoo", 80, 70),
                ("zoo_reversed", 80, 70), ("quad", 72, 72)]


def clamp_box(uv, w, h):
    """the texels the library's box of a triangle holds when it is no sliver (rpt_amd/csrc/lightmap_plan.h clamp_range): one
    more on either side than floor and ceil of the texel-space extent give -> (H, W) bool"""
    ax, ay = uv[:, 0] * float(w), uv[:, 1] * float(h)
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    return ((x >= np.floor(ax.min()) - 1) & (x < np.ceil(ax.max()) + 1) & (y >= np.floor(ay.min()) - 1) & (y < np.ceil(ay.max()) + 1))


# Slivers found by a search made once: three vertices on the uv diagonal, each coordinate within an ulp of it.  Their areas
# are tiny but not zero, and the header's ROUNDED edge tests cover texels along their line beyond their vertices — outside
# any box around the triangle (the first: area 2.9e-15 on a 16 x 16 map, where it covers texel (10, 10), 1.9 texels past its
# furthest vertex).  Per map size, because a vertex's rounding is the map's
def _hex(rows):
    return [[float.fromhex(c) for c in v] for v in rows]


SLIVERS = {
    (16, 16): [_hex([["0x1.650a87471b06cp-2", "0x1.650a87471b06cp-2"], ["0x1.4c5d63b09e87dp-2", "0x1.4c5d63b09e87cp-2"],
                     ["0x1.1314877c90929p-1", "0x1.1314877c90929p-1"]]),
               _hex([["0x1.d22fe0f4e3b35p-4", "0x1.d22fe0f4e3b34p-4"], ["0x1.04a8b2820dfe9p-2", "0x1.04a8b2820dfe9p-2"],
                     ["0x1.89b0dbe0a58dcp-3", "0x1.89b0dbe0a58dcp-3"]]),
               _hex([["0x1.d05b817298853p-3", "0x1.d05b817298853p-3"], ["0x1.19b2dbd082a03p-2", "0x1.19b2dbd082a03p-2"],
                     ["0x1.d03962aed9dd5p-4", "0x1.d03962aed9dd3p-4"]])],
    (13, 7): [_hex([["0x1.cfdf4f506dc6cp-4", "0x1.cfdf4f506dc6bp-4"], ["0x1.30659065a4c10p-2", "0x1.30659065a4c10p-2"],
                    ["0x1.8a21e810e4801p-9", "0x1.8a21e810e4801p-9"]]),
              _hex([["0x1.3cc7c3ac4c831p-1", "0x1.3cc7c3ac4c831p-1"], ["0x1.2d3dabbe0c7f5p+0", "0x1.2d3dabbe0c7f4p+0"],
                    ["0x1.11bcf9fe48b26p+0", "0x1.11bcf9fe48b25p+0"]]),
              _hex([["-0x1.7054a42ad1100p-5", "-0x1.7054a42ad10ffp-5"], ["0x1.89753253e8301p-3", "0x1.89753253e8301p-3"],
                    ["-0x1.4d64fc1c10581p-8", "-0x1.4d64fc1c10581p-8"]])],
    (72, 72): [_hex([["0x1.1f7162b803789p-3", "0x1.1f7162b80378ap-3"], ["0x1.98dee18c9fd1dp-2", "0x1.98dee18c9fd1dp-2"],
                     ["0x1.7024e1353edfcp-2", "0x1.7024e1353edfcp-2"]]),
               _hex([["0x1.c80686755502dp-3", "0x1.c80686755502cp-3"], ["0x1.96fce6e7d1d3fp-2", "0x1.96fce6e7d1d3fp-2"],
                     ["0x1.3d61e652c7618p-3", "0x1.3d61e652c7617p-3"]]),
               _hex([["0x1.3748bf8d94d90p-2", "0x1.3748bf8d94d90p-2"], ["0x1.c76658c10d976p-2", "0x1.c76658c10d975p-2"],
                     ["0x1.a3d5d5669c9a8p-3", "0x1.a3d5d5669c9a6p-3"]])],
}


def sliver_chart(w, h):
    """the map's three slivers, then an honest triangle larger than the map, which owns what they leave"""
    return np.array(SLIVERS[(w, h)] + [ZOO[6]])


@functools.lru_cache(maxsize=None)
def triangles(chart, scene="cornell"):
    """(positions (n, 3, 3), normals (n, 3, 3) — no unit vectors —, uvs (n, 3, 2)) of a chart's triangles, read-only.  The
    reversed zoo is the zoo's triangles in reversed order, not new ones"""
    if chart.endswith("_reversed"):
        return tuple(np.ascontiguousarray(a[::-1]) for a in triangles(chart[:-len("_reversed")], scene))
    uvs = sliver_chart(*map(int, chart[len("slivers"):].split("x"))) if chart.startswith("slivers") else np.array(CHARTS[chart], dtype=np.float64)
    rs = np.random.RandomState(sum(map(ord, chart + scene)))
    lo, hi = BOXES[scene]
    pos = rs.uniform(lo, hi, (len(uvs), 3, 3))
    nrm = rs.standard_normal((len(uvs), 3, 3)) + np.array([0.0, 2.0, 0.0])
    for a in (pos, nrm, uvs):
        a.setflags(write=False)
    return pos, nrm, uvs


# ---- 1. the raster against the model
@pytest.mark.parametrize("flat", [False, True], ids=["normals", "flat"])
@pytest.mark.parametrize("chart,w,h", RASTER_CASES, ids=["%s-%dx%d" % c for c in RASTER_CASES])
def test_raster_is_the_models(chart, w, h, flat):
    pos, nrm, uvs = triangles(chart)
    normals = None if flat else nrm
    want = M.raw(pos, normals, uvs, w, h, offset=0.25)
    covers = M.coverage(uvs, w, h)[0]
    owned = want["owner"] >= 0
    # the case shows what it is there for — by the model alone
    assert owned.mean() >= 0.40, owned.mean()
    if (w, h) == (16, 16):
        if chart == "quad":
            assert int(owned.sum()) == 196 and (want["owner"][np.arange(1, 15), np.arange(1, 15)] == 0).all()
        else:
            k = {j: (j if chart == "zoo" else 6 - j) for j in range(7)}   # the zoo's triangle j in this case's order
            assert not covers[k[0]].any() and not covers[k[1]].any() and not covers[k[2]].any()   # zero area, NaN, outside
            assert M.coverage(uvs, w, h)[2][k[3]] < 0.0 and covers[k[3]].any()                    # mirrored, and covering
            assert (covers[k[3]] & covers[k[4]]).any()                                             # two overlapping charts
            assert covers[k[5]].any() and uvs[k[5]][:, 0].max() > 1.0                              # over the edge
            assert covers[k[6]].all() and owned.all()                                              # larger than the map
            assert set(want["owner"].ravel().tolist()) == ({3, 4, 5, 6} if chart == "zoo" else {0})
    got = gpu("cornell").bake_lightmap(pos, uvs, w, h, normals=normals, seed=SEED, offset=0.25, channels=RAW)
    assert sorted(got) == sorted(RAW_NAMES) and got["owner"].shape == (h, w) and got["position"].shape == (h, w, 3)
    assert differing(got, want) == []
    assert (got["barycentric"][~owned] == 0.0).all() and (got["owner"][~owned] == -1).all()


@pytest.mark.parametrize("flat", [False, True], ids=["normals", "flat"])
@pytest.mark.parametrize("w,h", sorted(SLIVERS))
def test_slivers_own_what_the_rounded_edge_tests_give_them(w, h, flat):
    """The rule is the rounded edge tests over EVERY texel of the map.  A triangle whose vertices are collinear up to rounding
    has a tiny area that is not zero, and all three rounded edge functions come out with the right sign at centres along its
    line far beyond its vertices: it covers texels outside any box around it, and as a low index it owns them.  (16 x 16 and
    13 x 7: the one-wavefront path; 72 x 72: a sliver's box is the whole map, 5 184 texels, the second launch's.)"""
    pos, nrm, uvs = triangles("slivers%dx%d" % (w, h))
    normals = None if flat else nrm
    want = M.raw(pos, normals, uvs, w, h, offset=0.25)
    covers, _, area = M.coverage(uvs, w, h)
    assert (area[:3] != 0.0).all() and (np.abs(area[:3]) < 1e-11).all()
    beyond = [covers[j] & ~clamp_box(uvs[j], w, h) for j in range(3)]
    assert all(b.any() for b in beyond)                                   # each covers texels outside its own box ...
    assert any((b & (want["owner"] == j)).any() for j, b in enumerate(beyond))   # ... and owns some
    if (w, h) == (16, 16):
        assert want["owner"][10, 10] == 0 and beyond[0][10, 10]
    assert (want["owner"] >= 0).all() and (want["owner"] == 3).mean() >= 0.40
    got = gpu("cornell").bake_lightmap(pos, uvs, w, h, normals=normals, seed=SEED, offset=0.25, channels=RAW)
    assert np.array_equal(got["owner"], want["owner"]) and M.same(got["barycentric"], want["barycentric"])
    # (a centre exactly on a sliver's line has e1 = e2 = e3 = 0: b = 0, m = 0 and n = 0 / 0 — "whatever that yields" is a NaN,
    # whose sign and payload are the machine's, not the arithmetic's: NaN against NaN, every other value on its bits)
    for k in ("position", "normal"):
        g, v = got[k], want[k]
        assert ((M.bits(g) == M.bits(v)) | (np.isnan(g) & np.isnan(v))).all(), k


def test_reversed_triangles_change_the_owner_and_nothing_else():
    """the same triangles in reversed order: a texel's owner is the new lowest index, and where that is the same triangle
    as before its barycentrics, gather point and normal are the same bits"""
    w, h = 16, 16
    g = gpu("cornell")
    pos, nrm, uvs = triangles("zoo")
    rpos, rnrm, ruvs = triangles("zoo_reversed")
    a = g.bake_lightmap(pos, uvs, w, h, normals=nrm, seed=SEED, offset=0.25, channels=RAW)
    b = g.bake_lightmap(rpos, ruvs, w, h, normals=rnrm, seed=SEED, offset=0.25, channels=RAW)
    covers = M.coverage(uvs, w, h)[0]
    lowest, highest = covers.argmax(axis=0), 6 - covers[::-1].argmax(axis=0)
    assert (a["owner"] == lowest).all() and (6 - b["owner"] == highest).all() and (lowest != highest).any()
    keeps = lowest == highest                 # texels one triangle alone covers
    assert keeps.any()
    for k in ("barycentric", "position", "normal"):
        assert M.same(a[k][keeps], b[k][keeps]), k
    # flat normals are Triangle.from_vertices', and differ from the given ones
    flat = g.bake_lightmap(pos, uvs, w, h, seed=SEED, offset=0.25, channels=RAW)
    assert M.same(flat["barycentric"], a["barycentric"]) and not M.same(flat["normal"], a["normal"])
    tri = rpt_amd.Triangle.from_vertices(*pos[6])         # (mesh.rs:27, in the host mirror)
    only6 = flat["normal"][a["owner"] == 6]
    assert M.same(only6, np.broadcast_to(np.array(tri.n1), only6.shape))


# ---- 2. the gathers against the calls that define them
def floor_chart(name):
    """a mesh that IS in the scene, untransformed — cornell's floor, wine_glass's table —: its triangles' rows, and uvs that
    lay its bounding rectangle in the two widest axes over [0.08, 0.92]^2 of the map"""
    scene = small_scenes.small(name)[0]
    rows = next(mesh.triangles for ob, child, chain, mesh in surface_model.meshes_of(scene)
                if ob == {"cornell": 0, "wine_glass": 1}[name] and child < 0 and chain == [None])
    rows = np.ascontiguousarray(rows)
    v = rows[:, :9].reshape(-1, 3, 3)
    ext = v.reshape(-1, 3).max(axis=0) - v.reshape(-1, 3).min(axis=0)
    ax = np.sort(np.argsort(ext)[1:])
    lo = v.reshape(-1, 3).min(axis=0)[ax]
    uvs = 0.08 + 0.84 * (v[:, :, ax] - lo) / ext[ax]
    return rows, np.ascontiguousarray(uvs)


@functools.lru_cache(maxsize=None)
def gather_case(name, kind):
    """-> (the call's keyword arguments, its full result) — computed once, shared, read-only"""
    if kind == "synthetic":
        pos, nrm, uvs = triangles("zoo", name)
        kw = dict(triangles=pos, normals=nrm, uvs=uvs, width=13, height=7, offset=0.0, stream_base=1000)
    else:
        rows, uvs = floor_chart(name)
        off = 1e-3 * float(np.abs(rows[:, :9]).max())
        kw = dict(triangles=rows, normals=None, uvs=uvs, width=13, height=7, offset=off, stream_base=5)
    kw.update(samples=SAMPLES, max_bounces=BOUNCES, seed=SEED, sample_index_base=3, max_distance=float("inf"))
    out = bake(gpu(name), kw, channels=ALL)
    for a in out.values():
        a.setflags(write=False)
    return kw, out


def bake(g, kw, **more):
    kw = dict(kw, **more)
    return g.bake_lightmap(kw.pop("triangles"), kw.pop("uvs"), kw.pop("width"), kw.pop("height"), **kw)


@pytest.mark.parametrize("kind", ["synthetic", "mesh"])
@pytest.mark.parametrize("name", SCENES)
def test_gathers_are_bake_probes_and_bake_ao_at_the_texels(name, kind):
    g = gpu(name)
    kw, out = gather_case(name, kind)
    owned = out["owner"] >= 0
    assert owned.mean() >= 0.40
    if kind == "mesh":
        assert not owned.all()                                   # ... and gutters, which hold +0.0
    ids = (kw["stream_base"] + np.arange(owned.size, dtype=np.uint32).reshape(owned.shape))[owned]
    p, n = np.ascontiguousarray(out["position"][owned]), np.ascontiguousarray(out["normal"][owned])
    want = g.bake_probes(p, n, kind=_abi.RPT_PROBE_IRRADIANCE, samples=SAMPLES, max_bounces=BOUNCES, seed=SEED,
                         sample_index_base=3, streams=ids)
    assert M.same(out["irradiance"][owned], want)
    want_ao = g.bake_ao(p, n, samples=SAMPLES, seed=SEED, sample_index_base=3, streams=ids)
    assert M.same(out["ao"][owned], want_ao)
    assert M.same(out["irradiance"][~owned], np.zeros((int((~owned).sum()), 3))) and M.same(out["ao"][~owned], np.zeros(int((~owned).sum())))
    if kind == "mesh":
        assert (out["irradiance"] > 0.0).any()                    # light reaches the lifted texels of a surface of the scene
        assert ((out["ao"][owned] >= 0.0) & (out["ao"][owned] <= 1.0)).all()
    # a finite reach is RptAoQuery's max_distance
    reach = 0.3 * float(np.abs(p).max())
    near = bake(g, kw, channels=AO, max_distance=reach)["ao"]
    assert M.same(near[owned], g.bake_ao(p, n, samples=SAMPLES, seed=SEED, sample_index_base=3, streams=ids, max_distance=reach))


def test_a_map_of_many_blocks_in_pieces(monkeypatch):
    """40 x 30 texels, every one owned: the texel pass, the scan and the scatter over several blocks, in three pieces of
    which the last is partial — against the defining calls over the whole map at once"""
    g = gpu("cornell")
    pos, nrm, uvs = triangles("zoo")
    monkeypatch.setenv("RPTGPU_LIGHTMAP_PIECE", "500")
    out = g.bake_lightmap(pos, uvs, 40, 30, normals=nrm, samples=4, max_bounces=2, seed=SEED, stream_base=7, channels=ALL)
    assert differing(out, M.raw(pos, nrm, uvs, 40, 30)) == [] and (out["owner"] >= 0).all()
    ids = 7 + np.arange(1200, dtype=np.uint32)
    p, n = out["position"].reshape(-1, 3), out["normal"].reshape(-1, 3)
    assert M.same(out["irradiance"].reshape(-1, 3), g.bake_probes(p, n, kind=_abi.RPT_PROBE_IRRADIANCE, samples=4, max_bounces=2,
                                                                   seed=SEED, streams=ids))
    assert M.same(out["ao"].reshape(-1), g.bake_ao(p, n, samples=4, seed=SEED, streams=ids))


# ---- 3. independence, each to the bit
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("piece", [1, 7, 64])
def test_pieces_do_not_change_a_bit(name, piece, monkeypatch):
    kw, want = gather_case(name, "synthetic")
    monkeypatch.setenv("RPTGPU_LIGHTMAP_PIECE", str(piece))   # (13 x 7 = 91 texels: 91, 13 and 2 pieces, the last one partial)
    assert differing(bake(gpu(name), kw, channels=ALL), want) == []


@pytest.mark.parametrize("name", SCENES)
def test_stream_base_is_the_rows_of_a_taller_map(name):
    """rows 2..3 of a 16 x 8 map baked on their own as a 16 x 2 map: the same chart moved down by two rows — v' = (v * 8 - 2) /
    2, and the chart is one whose texel-space vertices are small integers in both maps, so every edge function is exact and
    the same number in both —, stream_base moved on by two rows: the texels' stream ids coincide, and with them every bit"""
    g = gpu(name)
    pos, nrm, _ = triangles("quad", name)
    tall = np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]])       # texel space (0, 0) .. (16, 8)
    part = np.array([[[0.0, -1.0], [1.0, -1.0], [1.0, 3.0]], [[0.0, -1.0], [1.0, 3.0], [0.0, 3.0]]])    # (0, -2) .. (16, 6)
    kw = dict(normals=nrm, samples=SAMPLES, max_bounces=BOUNCES, seed=SEED, offset=0.125, channels=ALL)
    a = g.bake_lightmap(pos, tall, 16, 8, stream_base=40, **kw)
    b = g.bake_lightmap(pos, part, 16, 2, stream_base=40 + 2 * 16, **kw)
    assert (a["owner"] >= 0).all() and set(a["owner"].ravel().tolist()) == {0, 1} and set(b["owner"].ravel().tolist()) == {0, 1}
    assert differing(b, {k: v[2:4] for k, v in a.items()}) == []
    other = g.bake_lightmap(pos, part, 16, 2, stream_base=40, **kw)                                      # (other streams: other bits)
    assert differing(other, b) == ["ao", "irradiance"] or differing(other, b) == ["irradiance"]


@pytest.mark.parametrize("name", SCENES)
def test_routes_do_not_change_a_bit(name):
    kw, want = gather_case(name, "synthetic")
    g = gpu(name)
    assert differing(bake(g, kw, channels=ALL, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL), want) == []
    if _abi.rays_persistent_supported():
        assert differing(bake(g, kw, channels=ALL, flags=_abi.RPT_FLAG_RAYS_PERSISTENT), want) == []
    with pytest.raises(rpt_amd.RptGpuError, match="RPT_FLAG_PERSISTENT"):
        bake(g, kw, channels=ALL, flags=_abi.RPT_FLAG_PERSISTENT)


@pytest.mark.parametrize("name", SCENES)
def test_device_tensors_give_the_host_calls_result(name):
    kw, want = gather_case(name, "synthetic")
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.array(kw[k])).to(dev) for k in ("triangles", "normals", "uvs")}
    got = bake(gpu(name), dict(kw, **t), channels=ALL, dilate=1)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values())
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, bake(gpu(name), kw, channels=ALL, dilate=1)) == []
    # a Mesh's rows, positions and normals in one tensor
    rows = torch.cat([t["triangles"].reshape(-1, 9), t["normals"].reshape(-1, 9)], dim=1)
    got = bake(gpu(name), dict(kw, triangles=rows, normals=None, uvs=t["uvs"]), channels=ALL)
    assert differing({k: v.cpu().numpy() for k, v in got.items()}, want) == []


def test_a_subset_of_channels_is_the_full_calls_and_unnamed_arrays_are_untouched():
    name = "cornell"
    kw, want = gather_case(name, "synthetic")
    g = gpu(name)
    for ch, names in ((IRR, ["irradiance"]), (AO | POS, ["ao", "position"]), (OWNER, ["owner"]), (NRM | BARY, ["barycentric", "normal"]),
                      (IRR | AO | OWNER, ["ao", "irradiance", "owner"])):
        got = bake(g, kw, channels=ch)
        assert sorted(got) == names and differing(got, want, names) == []
    # through the C entry point: every array handed over, two channels named — the others keep their sentinel
    import ctypes as C
    n = kw["width"] * kw["height"]
    outs = {"irradiance": np.full((n, 3), 7.0), "ao": np.full(n, 7.0), "owner": np.full(n, 7, dtype=np.int32),
            "barycentric": np.full((n, 3), 7.0), "position": np.full((n, 3), 7.0), "normal": np.full((n, 3), 7.0)}
    q = _abi.RptLightmapQuery()
    q.struct_size, q.channels, q.width, q.height = C.sizeof(q), AO | BARY, kw["width"], kw["height"]
    q.samples, q.max_bounces, q.stream_base, q.seed, q.sample_index_base = SAMPLES, BOUNCES, kw["stream_base"], SEED, 3
    q.offset, q.max_distance = kw["offset"], float("inf")
    a = _abi.RptLightmapArrays()
    a.struct_size = C.sizeof(a)
    types = dict(_abi.RptLightmapArrays._fields_)
    for k, v in outs.items():
        setattr(a, k, v.ctypes.data_as(types[k]))
    PD = C.POINTER(C.c_double)
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(PD)
    pos, nrm, uvs = (np.ascontiguousarray(kw[k]) for k in ("triangles", "normals", "uvs"))
    _abi.check(g.lib.rptgpu_bake_lightmap(g.handle, len(pos), p(pos), p(nrm), p(uvs), C.byref(q), C.byref(a)), g.handle)
    assert M.same(outs["ao"].reshape(want["ao"].shape), want["ao"]) and M.same(outs["barycentric"].reshape(want["barycentric"].shape), want["barycentric"])
    assert all((outs[k] == 7).all() for k in ("irradiance", "owner", "position", "normal"))


def test_after_set_objects_the_bake_is_a_fresh_handles():
    scene = small_scenes.small("cornell")[0]
    g = GpuScene(scene, 0)
    kw, before = gather_case("cornell", "mesh")
    assert differing(bake(g, kw, channels=ALL), before) == []
    moved = small_scenes.small("cornell")[0]
    moved.objects[6] = rpt_amd.Object(rpt_amd.cube().scale((165.0, 165.0, 165.0)).rotate_y(0.3).translate((300.0, 82.5, 250.0))) \
        .material(rpt_amd.Material.diffuse(rpt_amd.hex_color(0xAAAAAA)))
    g.set_objects([6], [moved.objects[6]])
    got = bake(g, kw, channels=ALL)
    assert differing(got, bake(GpuScene(moved, 0), kw, channels=ALL)) == []
    assert differing(got, before, ["irradiance"]) == ["irradiance"]   # (the update is seen)


# ---- 4. dilation
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("rounds", [0, 1, 3, 13])
def test_dilation_is_the_models_over_the_calls_own_output(name, rounds):
    """13 = max(W, H): more rounds than the 13 x 7 map has gutters to fill"""
    kw, plain = gather_case(name, "mesh")
    owned = plain["owner"] >= 0
    assert 0.40 <= owned.mean() < 1.0
    got = bake(gpu(name), kw, channels=ALL, dilate=rounds)
    assert M.same(got["irradiance"], M.dilate(plain["irradiance"], owned, rounds)[0])
    assert M.same(got["ao"], M.dilate(plain["ao"], owned, rounds)[0])
    assert differing(got, plain, RAW_NAMES) == []                       # the raw channels are never dilated
    if rounds:
        assert not M.same(got["irradiance"], plain["irradiance"])
    if rounds == 13:
        assert (got["irradiance"][~owned].max(axis=1) > 0.0).all()       # every gutter texel is filled by then
    # one channel alone dilates as it does beside the other
    assert M.same(bake(gpu(name), kw, channels=AO, dilate=rounds)["ao"], got["ao"])


# ---- 5. no triangles
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_triangles_leave_every_texel_unowned(device):
    g = gpu("cornell")
    empty = np.zeros((0, 3, 3)), np.zeros((0, 3, 2))
    if device:
        empty = tuple(torch.from_numpy(a).to(torch.device("cuda", 0)) for a in empty)
    got = g.bake_lightmap(empty[0], empty[1], 5, 3, samples=SAMPLES, max_bounces=BOUNCES, seed=SEED, dilate=2, channels=ALL)
    got = {k: (v.cpu().numpy() if device else v) for k, v in got.items()}
    assert (got["owner"] == -1).all() and got["owner"].shape == (3, 5)
    for k in ("irradiance", "ao", "barycentric", "position", "normal"):
        assert M.same(got[k], np.zeros(got[k].shape)), k
