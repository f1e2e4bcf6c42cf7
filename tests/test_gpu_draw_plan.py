"""A hit's draws by Philox block (kernels/paths_shade.inc hit_draws, RPT_DRAW_PLAN) on a real MI355X.  The stream is
random-access, so the planned form may change WHEN a block is computed and never which draw feeds which value:
(1) hit_draws as built (rptgpu_eval_math's function 12) and the sequence of single next_u64 calls (function 13) give, for
2^16 elements, the fields, the final draw counter and the cached half of a Philox4x32-10 model written here in numpy,
bit for bit — over both parities of the counter, every f of gen_bool's cases, both values of sf, light meshes of one, two
and three triangles, a constructed zone that makes index draws fail (the wave's sequential branch), and lanes with many
redraws of either pair; (2) Cornell frames, one with a white metal box (f == 1.0: no gen_bool draw) beside diffuse lanes,
equal the oracle's bit for bit with its ray counts; (3) a library built with -DRPT_DRAW_PLAN=0
(scripts/build_variant.sh drawplan0 "-DRPT_DRAW_PLAN=0"), when there is one, gives the same frames and counts."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rpt_amd import Camera, GpuScene, Light, Material, Object, Scene, _abi, cube, hex_color, make_params, polygon, scenes  # noqa: E402

gpu = pytest.mark.gpu

AB_LIB = os.path.join(ROOT, "rpt_amd", "lib", "librptgpu_drawplan0.so")  # scripts/build_variant.sh drawplan0 "-DRPT_DRAW_PLAN=0"
PERSISTENT = _abi.RPT_FLAG_PERSISTENT
FUSED = "shadow and bounce rays in one query"
FN_AS_BUILT, FN_SEQUENCE = 12, 13

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
S32 = U64(32)


# ---- the model: Philox4x32-10 (key = the seed's halves, counter = pixel, the sample's halves, the block) and the
# reference's sequence of draws on it, draw k = half k & 1 of block k >> 1
def philox(seed, pixel, sample, block):
    k0, k1 = seed & M32, seed >> S32
    c0, c1, c2, c3 = pixel & M32, sample & M32, sample >> S32, block & M32
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return (c1 << S32) | c0, (c3 << S32) | c2


def draw(el, k):
    lo, hi = philox(el["seed"], el["pixel"], el["sample"], k >> U64(1))
    return np.where((k & U64(1)) != 0, hi, lo)


def mul_hi(v, n):  # the high word of v * n, n < 2^32
    return ((v >> S32) * n + (((v & M32) * n) >> S32)) >> S32


def unit(v):  # rand's Standard f64
    return (v >> U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def pm1(v):  # gen_range(-1.0, 1.0) on the 52-bit mantissa
    return ((v >> U64(12)) | U64(0x3FF0000000000000)).view(np.float64) - 1.0


def model(el):
    """the nine output words of every element ([elements][9] u64) and what the sequence went through: index draws
    rejected, (u, v) pairs rejected, +-1 pairs rejected, the counter in front of gen_bool"""
    n_el = len(el["seed"])
    d = el["start"].copy()
    one = U64(1)
    out = np.zeros((n_el, 9), dtype=U64)
    stats = {k: np.zeros(n_el, dtype=np.int64) for k in ("index_rejects", "uv_rejects", "pm_rejects")}
    with np.errstate(over="ignore"):
        todo = np.ones(n_el, dtype=bool)
        while todo.any():  # gen_index_zone
            v = draw(el, d)
            ok = v * el["prims"] <= el["zone"]
            out[:, 0] = np.where(todo & ok, mul_hi(v, el["prims"]), out[:, 0])
            d += todo.astype(U64)
            stats["index_rejects"] += todo & ~ok
            todo &= ~ok
        todo = np.ones(n_el, dtype=bool)
        while todo.any():  # (u, v) until u + v <= 1
            a, b = draw(el, d), draw(el, d + one)
            ok = unit(a) + unit(b) <= 1.0
            out[:, 1], out[:, 2] = np.where(todo, a, out[:, 1]), np.where(todo, b, out[:, 2])
            d += todo.astype(U64) * U64(2)
            stats["uv_rejects"] += todo & ~ok
            todo &= ~ok
        stats["counter_at_gen_bool"] = d.copy()
        out[:, 3] = one << U64(63)
        sf = el["sf"]
        f = el["f"]
        takes = sf & (f != 1.0)  # gen_bool: no draw when f == 1.0
        p_int = np.where(f != 1.0, f, 0.0) * 18446744073709551616.0
        spec = sf & np.where(takes, draw(el, d) < p_int.astype(U64), True)
        d += takes.astype(U64)
        out[:, 3] = np.where(spec, draw(el, d), out[:, 3])
        d += spec.astype(U64)
        out[:, 6] = spec
        todo = sf.copy()
        while todo.any():  # unit_circle / unit_disc
            a, b = draw(el, d), draw(el, d + one)
            s = pm1(a) * 2.0 + -1.0
            t = pm1(b) * 2.0 + -1.0
            ssum = s * s + t * t
            ok = np.where(spec, ssum < 1.0, ssum <= 1.0)
            out[:, 4], out[:, 5] = np.where(todo, a, out[:, 4]), np.where(todo, b, out[:, 5])
            d += todo.astype(U64) * U64(2)
            stats["pm_rejects"] += todo & ~ok
            todo &= ~ok
    out[:, 7] = d
    out[:, 8] = np.where((d & one) != 0, draw(el, d), U64(0))
    return out, stats


# ---- the elements
N_ELEMENTS = 1 << 16
F_CASES = (0.0, 0.232, float(np.nextafter(1.0, 0.0)), 1.0)
N_FALLBACK = 4096  # the last waves: a constructed zone, so that index draws fail
_elements = {}


def true_zone(n):
    return (1 << 64) - 1 - ((1 << 64) - n) % n


def elements():
    """every combination of (start counter, f, sf, triangles, the form with the material's table) in turn, so that a wave
    holds all of them side by side; seeds, pixels and samples from a fixed generator, which model() below shows to hold the
    cases with many redraws; the elements behind 3/4 of the set at large counters; the last N_FALLBACK with a zone of
    2^63 in two lanes of three (an index draw then fails in one of two)"""
    if _elements:
        return _elements
    rs = np.random.RandomState(20240611)
    e = np.arange(N_ELEMENTS)
    c = e % 192
    start = (c % 4).astype(U64)
    f = np.array(F_CASES)[(c // 4) % 4]
    sf = ((c // 16) % 2).astype(bool)
    prims = (1 + (c // 32) % 3).astype(U64)
    table = ((c // 96) % 2).astype(U64)
    far = e >= N_ELEMENTS * 3 // 4
    start = np.where(far, rs.randint(0, 1 << 31, N_ELEMENTS).astype(U64), start)
    zone = np.array([true_zone(int(n)) for n in prims], dtype=U64)
    low = (e >= N_ELEMENTS - N_FALLBACK) & (e % 3 != 0)
    zone = np.where(low, U64(1 << 63), zone)
    _elements.update(
        seed=rs.randint(0, 1 << 63, N_ELEMENTS).astype(U64) * U64(2) + rs.randint(0, 2, N_ELEMENTS).astype(U64),
        pixel=rs.randint(0, 1 << 32, N_ELEMENTS).astype(U64), sample=rs.randint(0, 1 << 40, N_ELEMENTS).astype(U64),
        start=start, prims=prims, zone=zone, f=f, sf=sf, table=table, constructed_zone=low)
    return _elements


def input_words(el):
    w = np.zeros((N_ELEMENTS, 9), dtype=U64)
    w[:, 0], w[:, 1], w[:, 2], w[:, 3], w[:, 4], w[:, 5] = el["seed"], el["pixel"], el["sample"], el["start"], el["prims"], el["zone"]
    w[:, 6] = el["f"].view(U64)
    w[:, 7] = el["sf"].astype(U64) + U64(2) * el["table"]
    return w.reshape(-1).view(np.float64)


def test_the_model_on_known_blocks():
    """Random123's known answers for Philox4x32-10: the model's block function is the published one"""
    def block(c0, c1, c2, c3, k0, k1):
        a = [np.array([v], dtype=U64) for v in ((k1 << 32) | k0, c0, (c2 << 32) | c1, c3)]
        lo, hi = philox(*a)
        return [int(lo[0]) & 0xFFFFFFFF, int(lo[0]) >> 32, int(hi[0]) & 0xFFFFFFFF, int(hi[0]) >> 32]

    assert block(0, 0, 0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert block(*([0xFFFFFFFF] * 6)) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert block(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_the_elements_hold_every_case():
    """what the set must contain, by the model — so that the comparison below cannot pass by leaving a case out"""
    el = elements()
    ref, st = model(el)
    odd_b = (st["counter_at_gen_bool"] & U64(1)) != 0
    spec = ref[:, 6] != 0
    regular = ~el["constructed_zone"]
    for s in range(4):  # the start counters: both parities, with and without a cached half
        assert (el["start"] == s).sum() >= 1000
    for fv in F_CASES:
        for sfv in (False, True):
            for n in (1, 2, 3):
                for tb in (0, 1):
                    assert ((el["f"] == fv) & (el["sf"] == sfv) & (el["prims"] == n) & (el["table"] == tb) & regular).sum() >= 100
    assert F_CASES[2] < 1.0 and F_CASES[2] * 18446744073709551616.0 == 18446744073709551616.0 - 2048.0
    assert (ref[regular, 0] < el["prims"][regular]).all() and (ref[el["prims"] == 3, 0] == 2).any()
    # the sequential branch: index draws that fail, beside lanes of the same wave whose draw is accepted
    assert (st["index_rejects"][regular] == 0).all()
    assert (st["index_rejects"][~regular] >= 1).sum() >= 500 and (st["index_rejects"] >= 3).sum() >= 10
    tail = st["index_rejects"][N_ELEMENTS - N_FALLBACK:].reshape(-1, 64)
    assert ((tail > 0).any(axis=1) & (tail == 0).any(axis=1)).all()
    # redraws: long runs of either pair, at both parities of the counter the hit starts at
    for parity in (0, 1):
        at = (el["start"] & U64(1)) == parity
        assert (st["uv_rejects"][at & regular] >= 6).sum() >= 50
        assert (st["uv_rejects"][at & regular] == 0).sum() >= 1000  # ... and lanes whose first pair is kept
        assert (st["pm_rejects"][odd_b == bool(parity)] >= 3).sum() >= 20
        for sp in (False, True):  # spec and non-spec lanes of both parities in front of gen_bool, with and without its draw
            assert (el["sf"] & (spec == sp) & (odd_b == bool(parity)) & (el["f"] != 1.0)).sum() >= 500
        assert (el["sf"] & spec & (odd_b == bool(parity)) & (el["f"] == 1.0)).sum() >= 500
    assert not spec[~el["sf"]].any() and (ref[~el["sf"], 3] == U64(1 << 63)).all() and (ref[~el["sf"], 4:6] == 0).all()
    assert ((ref[:, 7] & U64(1)) != 0).sum() >= 1000 and (ref[:, 8] != 0).sum() >= 1000  # cached halves to compare


@pytest.fixture(scope="module")
def handle():
    g = GpuScene(scenes.sphere_scene()[0], 0)
    yield g
    g.close()


@gpu
def test_draws_equal_the_sequence_and_the_model(handle):
    el = elements()
    ref, _ = model(el)
    x = input_words(el)
    built = handle.eval_math(FN_AS_BUILT, x).view(U64).reshape(-1, 9)
    seq = handle.eval_math(FN_SEQUENCE, x).view(U64).reshape(-1, 9)
    names = ("tri", "a", "b", "th", "qa", "qb", "spec", "draw", "cached half")
    for got, what in ((seq, "the next_u64 sequence"), (built, "hit_draws as built")):
        bad = np.nonzero((got != ref).any(axis=1))[0]
        assert len(bad) == 0, (what, len(bad), [(int(i), [names[k] for k in np.nonzero(got[i] != ref[i])[0]]) for i in bad[:8]])
    assert (built == seq).all()


@gpu
def test_draw_entries_refuse_elements_whose_loops_could_not_end(handle):
    import rpt_amd
    x = input_words(elements())[:9].copy()
    for word, value in ((5, U64(0)), (4, U64(0)), (6, np.float64(1.5).view(U64)), (3, U64(1 << 31))):
        w = x.view(U64).copy()
        w[word] = value
        with pytest.raises(rpt_amd.RptGpuError):
            handle.eval_math(FN_AS_BUILT, w.view(np.float64))
    assert (handle.eval_math(FN_AS_BUILT, x[:8]) == 0.0).all()  # no whole element: nothing runs


# ---- frames: name -> (scene, width, height, bounces, spp, seed)
FRAMES = {
    "cornell_96x64": ("cornell", 96, 64, 8, 4, 311),
    "cornell_33x17": ("cornell", 33, 17, 8, 4, 312),  # a partial last wave
    "metal_box_96x64": ("metal_box", 96, 64, 8, 4, 313),
}
METAL = Material.metallic_(hex_color(0xFFFFFF), 0.1)
_refs = {}
_here = {}


def lobe_probability(m):
    """sample_f's f (material.rs), in the oracle's operation order"""
    f0 = ((m.index - 1.0) / (m.index + 1.0)) ** 2
    mean = ((m.color[0] + m.color[1]) + m.color[2]) / 3.0
    f = (1.0 - m.metallic) * f0 + m.metallic * mean
    return f * (1.0 - 0.2) + 1.0 * 0.2


def metal_box_cornell():
    """scenes.cornell() with its tall box of white metal: f == 1.0 there, beside the diffuse walls' f < 1.0"""
    scene = Scene()
    camera = Camera(eye=(278.0, 273.0, -800.0), direction=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0), fov=0.686)
    white, red, green = (Material.diffuse(hex_color(c)) for c in (0xAAAAAA, 0xBC0000, 0x00BC00))
    walls = [
        ([(0.0, 0.0, 0.0), (0.0, 0.0, 559.2), (556.0, 0.0, 559.2), (556.0, 0.0, 0.0)], white),
        ([(0.0, 548.9, 0.0), (556.0, 548.9, 0.0), (556.0, 548.9, 559.2), (0.0, 548.9, 559.2)], white),
        ([(0.0, 0.0, 559.2), (0.0, 548.9, 559.2), (556.0, 548.9, 559.2), (556.0, 0.0, 559.2)], white),
        ([(556.0, 0.0, 0.0), (556.0, 0.0, 559.2), (556.0, 548.9, 559.2), (556.0, 548.9, 0.0)], red),
        ([(0.0, 0.0, 0.0), (0.0, 548.9, 0.0), (0.0, 548.9, 559.2), (0.0, 0.0, 559.2)], green),
    ]
    for pts, m in walls:
        scene.add(Object(polygon(pts)).material(m))
    two_pi = 2.0 * math.pi
    scene.add(Object(cube().scale((165.0, 330.0, 165.0)).rotate_y(two_pi * (-253.0 / 360.0)).translate((368.0, 165.0, 351.0)))
              .material(METAL))
    scene.add(Object(cube().scale((165.0, 165.0, 165.0)).rotate_y(two_pi * (-197.0 / 360.0)).translate((185.0, 82.5, 169.0)))
              .material(white))
    light = polygon([(343.0, 548.8, 227.0), (343.0, 548.8, 332.0), (213.0, 548.8, 332.0), (213.0, 548.8, 227.0)])
    scene.add(Light.Object(Object(light).material(Material.light(hex_color(0xFFFEFA), 100.0))))
    return scene, camera


def frame_inputs(name):
    src, w, h, b, spp, seed = FRAMES[name]
    scene, cam = scenes.cornell()[:2] if src == "cornell" else metal_box_cornell()
    return scene, cam, make_params(w, h, b, spp, seed=seed, flags=PERSISTENT)


def reference(oracle, name):
    """the oracle's frame and counters of a frame, rendered once"""
    if name not in _refs:
        scene, cam, p = frame_inputs(name)
        _refs[name] = oracle.OracleScene(scene).render(cam, p, threads=0, counters=True)
    return _refs[name]


def render_frames(launch_lines=None):
    """every frame of FRAMES with this process's library: the f64 frame (render_batch), the f32 frame of
    render_batch_reduce and the latter's ray counts"""
    out = {}
    for name in FRAMES:
        scene, cam, p = frame_inputs(name)
        g = GpuScene(scene, 0)
        try:
            out[name] = g.render_batch(cam, p)
            g.reset_stats()
            out[name + "_reduce"] = g.render_batch_reduce(cam, p, root=0)
            st = g.stats()
            out[name + "_rays"] = np.array([st.extend_rays, st.shadow_rays, st.kernel_launches[_abi.RPT_K_PATHS]], dtype=np.uint64)
            if launch_lines is not None:
                launch_lines(name, g, cam)
        finally:
            g.close()
    return out


def frames_here():
    if not _here:
        _here.update(render_frames())
    return _here


def test_the_metal_box_takes_no_gen_bool_draw():
    assert lobe_probability(METAL) == 1.0 and lobe_probability(Material.diffuse(hex_color(0xAAAAAA))) < 1.0


@gpu
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_equal_the_oracles(oracle, capfd, name):
    ref, cnt = reference(oracle, name)
    got = frames_here()
    img, red, rays = got[name], got[name + "_reduce"], got[name + "_rays"]
    assert np.isfinite(img).all() and img.max() > 0.0
    assert (img.view(np.int64) == ref.view(np.int64)).all(), (name, np.abs(img - ref).max())
    assert (red.view(np.int32) == ref.astype(np.float32).ravel().view(np.int32)).all(), name
    assert (int(rays[0]), int(rays[1])) == (cnt["closest_rays"], cnt["shadow_rays"]), (name, rays, cnt)
    assert int(rays[2]) >= 1
    # the frame ran through the kernel whose hits take their draws first
    scene, cam, p = frame_inputs(name)
    g = GpuScene(scene, 0)
    try:
        capfd.readouterr()
        os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
        try:
            g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
        finally:
            del os.environ["RPTGPU_PRINT_LAUNCH"]
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths<")]
        assert lines and all(FUSED in ln for ln in lines), lines
    finally:
        g.close()


@gpu
@pytest.mark.skipif(not os.path.exists(AB_LIB), reason="no library built with -DRPT_DRAW_PLAN=0 (scripts/build_variant.sh drawplan0)")
def test_library_without_the_plan_gives_the_same_frames(tmp_path):
    path = str(tmp_path / "old.npz")
    env = dict(os.environ, RPTGPU_LIB=AB_LIB)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    old, new = np.load(path), frames_here()
    for name in FRAMES:
        assert (old[name].view(np.int64) == new[name].view(np.int64)).all(), name
        assert (old[name + "_reduce"].view(np.int32) == new[name + "_reduce"].view(np.int32)).all(), name
        assert tuple(old[name + "_rays"]) == tuple(new[name + "_rays"]), name


if __name__ == "__main__":
    np.savez(sys.argv[1], **render_frames())
