"""Sampled shapes and objects under sheared, mirrored, matrix and singular placements on the GPU, held to the oracle bit for
bit (tests/placement_cases.py has the placements, lamp shapes and scenes; tests/test_placements_host.py holds the oracle to
the reference's text and shows that every signal compared here is there).  Transformed::sample reads transform, linear and
scale of a placement, which no intersection reads: at top level, in a group child's record and at every level of a nested
group's chain (kernels/sampling.inc).  Under the placements here a transposed matrix, a sign or an fmax on the pdf shows:
the lamps emit NEGATIVE light under a negative determinant and NaN under a singular one, as the reference's do.

1. rptgpu_bake_direct is the model's fold of the oracle's illuminate (tests/test_gpu_direct.py's assertion) for every lamp
   shape under every placement, the lamp moved between placements by set_lights on one handle per geometry;
2. a room's frames under 0, PERSISTENT and WAVEFRONT with the oracle's ray counts — the fused persistent kernel shades these
   hits in its sequence branch (a light that is no untransformed mesh), and the launch line must name it;
3. a yard of placed objects of every kind: closest hits and frames on every route;
4. the fused kernel's cube-normal tables under two negative determinants;
5. live updates of a lamp's and of objects' placements.
NaN payloads are no part of the contract: a NaN equals a NaN (placement_cases.same)."""
import functools
import os

import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from oracle import oracle_ffi as O
from rpt_amd import GpuScene, _abi, make_params

import direct_cases as DC
import direct_model as DM
import placement_cases as PC

pytestmark = pytest.mark.gpu

GENERAL, PERSISTENT, WAVEFRONT = _abi.RPT_FLAG_GENERAL_TRAVERSAL, _abi.RPT_FLAG_PERSISTENT, _abi.RPT_FLAG_WAVEFRONT
FLAGS = [0, PERSISTENT, WAVEFRONT]
FLAG_IDS = ["default", "persistent", "wavefront"]
FUSED = "shadow and bounce rays in one query"
TABLES = "a hit's scene constants from the wave's tables"
SAMPLES = 33
N = PC.N_POINTS
same = PC.same


@functools.lru_cache(maxsize=None)
def fresh(name, placement):
    """a handle made from the room with its lamp in place, never updated"""
    return GpuScene(PC.room_case(name, placement)[0], 0)


@functools.lru_cache(maxsize=None)
def movable(name, geometry):
    """one handle per lamp geometry (a sphere, cube and monomial lamp: one per shape), its lamp moved by set_lights"""
    first = [p for p in PC.PLACEMENTS if PC.geometry(name, p) == geometry][0]
    return GpuScene(PC.room_case(name, first)[0], 0)


def moved_to(name, placement):
    g = movable(name, PC.geometry(name, placement))
    g.set_lights([0], PC.room_case(name, placement)[0].lights)
    return g


def closest_t(g):
    return lambda o, d: g.closest_hit(o, d)[0]


@functools.lru_cache(maxsize=None)
def direct_case(name, placement):
    """(out, the triples' details) as include/rpt_gpu_direct.h defines them for the room's points: the oracle's illuminate,
    the device's closest_hit (the rooms share their objects: the lamp is none), the model's fold — computed once, read-only"""
    pos, nrm, ids = PC.points("room")
    out, det = DM.direct(PC.room_case(name, placement)[0].lights, pos, nrm, SAMPLES, PC.BAKE_SEED, closest_t(fresh("sphere", "shear")),
                         streams=ids, illuminate=DC.oracle_illuminate, details=True)
    out.setflags(write=False)
    return out, det


def bake(g, key="room", flags=0):
    pos, nrm, ids = PC.points(key)
    return g.bake_direct(pos, nrm, samples=SAMPLES, seed=PC.BAKE_SEED, streams=ids, flags=flags)


# ---- 1. the direct bake is the model's fold, for every lamp shape under every placement
@pytest.mark.parametrize("flags", [0, GENERAL], ids=["routed", "general"])
@pytest.mark.parametrize("placement", PC.PLACEMENTS)
@pytest.mark.parametrize("name", PC.LAMPS)
def test_bake_direct_is_the_fold_of_illuminate_and_closest_hit(name, placement, flags):
    want, det = direct_case(name, placement)
    queued = int(((det["cosv"] > 0.0) & ~(det["c"] == 0.0).all(axis=1)).sum())  # the triples whose light can add something
    dead = (name, placement) == ("sphere", "singular")
    if dead:
        # the one case without a signal, by the call's definition: the sample point of a sphere under glm::inverse's zeros
        # is NaN, so is wi, and a light adds only where wi . n > 0 (test_placements_host says why no scene can change that)
        assert (want == 0.0).all() and queued == 0 and np.isnan(det["cosv"]).all()
    else:
        assert (want != 0.0).any() and 0.10 <= det["adds"].mean() <= 0.90
        sign = PC.leaf_sign(name, placement)
        lit = (want != 0.0).any(axis=1)
        assert np.isnan(want[lit]).any(axis=1).all() if sign == 0 else (np.sign(want[lit]) == sign).all()
    g = moved_to(name, placement)
    g.reset_stats()
    got = bake(g, flags=flags)
    assert got.dtype == np.float64 and got.shape == (N, 3)
    assert same(got, want), (np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).all(axis=1)), got, want)
    st = g.stats()
    assert st.shadow_rays == N * SAMPLES and st.shadow_rays_traced == queued and st.samples == 0
    assert dead or 0 < queued < st.shadow_rays  # (the lamp faces away from some point: its ray is never traced)
    assert st.kernel_launches[_abi.RPT_K_SHADOW] >= (0 if dead else 1) and st.kernel_launches[_abi.RPT_K_PATHS] == 0


# ---- 2. frames
FRAME_CASES = [(n, p) for n in PC.LAMPS for p in ("shear", "mirror", "matrix")] + \
              [(n, p) for n in ("sphere", "cube") for p in ("singular", "bottom_row")]
# what RPTGPU_PRINT_LAUNCH says of a room under RPT_FLAG_PERSISTENT.  Every lamp here is a light that is no untransformed
# mesh: the fused kernel shades its hits in the sequence branch (kernels/paths_loop.inc), and the line must name that
# kernel — a fallback cannot pass in its place.  The extended-shape build (a monomial lamp, a lamp that is a group of
# groups) has the same forms: scene_plan.h's flat plan does not ask which build runs it
LAUNCH = {name: ("rpt_paths<KdFlat>", FUSED) for name in PC.LAMPS}


def launch_lines(g, cam, capfd):
    capfd.readouterr()
    os.environ["RPTGPU_PRINT_LAUNCH"] = "1"
    try:
        g.render_batch(cam, make_params(16, 9, 2, 1, seed=1, flags=PERSISTENT))
    finally:
        del os.environ["RPTGPU_PRINT_LAUNCH"]
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rpt_paths")]
    print("\n".join(lines))
    return [ln for ln in lines if ln.startswith("rpt_paths<")]


def check(g, cam, ref, cnt, flags, bounces=PC.BOUNCES, tree_kids=False):
    """test_gpu_scene_consts.check: the frame's bits and the oracle's ray counts.  tree_kids: the scene has a group with tree
    children, which only the per-tree pipeline walks — RPT_FLAG_PERSISTENT is a request it cannot honour (test_gpu_parity's
    test_groups_with_tree_children_take_the_per_tree_pipeline_whatever_is_asked): the same frame, no persistent launch"""
    g.reset_stats()
    img = g.render_batch(cam, PC.params(bounces, flags))
    st = g.stats()
    if flags == PERSISTENT:
        assert (st.kernel_launches[_abi.RPT_K_PATHS] == 0) if tree_kids else (st.kernel_launches[_abi.RPT_K_PATHS] >= 1)
    bad = ~((img.view(np.int64) == ref.view(np.int64)) | (np.isnan(img) & np.isnan(ref))).all(axis=1)
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5], img[bad][:3], ref[bad][:3])
    assert st.extend_rays == cnt["closest_rays"], (st.extend_rays, cnt["closest_rays"])
    assert st.shadow_rays == cnt["shadow_rays"], (st.shadow_rays, cnt["shadow_rays"])
    return img


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("name,placement", FRAME_CASES)
def test_a_rooms_frames_are_the_oracles(name, placement, flags, capfd):
    scene, cam = PC.room_case(name, placement)
    ref, cnt = PC.room_frame(name, placement)
    g = fresh(name, placement)
    if flags == PERSISTENT:
        lines = launch_lines(g, cam, capfd)
        assert lines and all(all(word in ln for word in LAUNCH[name]) for ln in lines), lines
    check(g, cam, ref, cnt, flags)


# ---- 3. the yard: placed objects of every kind, two lights
HIT = _abi.RPT_HIT_T | _abi.RPT_HIT_NORMAL | _abi.RPT_HIT_OBJECT


@functools.lru_cache(maxsize=None)
def yard_gpu(variant):
    return GpuScene(PC.yard(variant)[0], 0)


@functools.lru_cache(maxsize=None)
def yard_hits(variant):
    o, d = PC.yard_rays()
    return O.OracleScene(PC.yard(variant)[0]).closest_hit(o, d)


@pytest.mark.parametrize("flags", [0, GENERAL], ids=["default", "general"])
@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_the_yards_closest_hits_are_the_oracles(variant, flags):
    o, d = PC.yard_rays()
    t0, n0, ob0 = yard_hits(variant)
    g = yard_gpu(variant)
    if flags:
        got = g.first_hits(o, d, channels=HIT, flags=flags)
        t1, n1, ob1 = got["t"], got["normal"], got["object"]
    else:
        t1, n1, ob1 = g.closest_hit(o, d)
    assert (ob0 == ob1).all(), np.flatnonzero(ob0 != ob1)
    assert same(t0, t1), np.flatnonzero(t0 != t1)
    assert same(n0, n1), np.flatnonzero((n0 != n1).any(axis=1))


@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_the_yards_frames_are_the_oracles(variant, flags):
    scene, cam = PC.yard(variant)
    check(yard_gpu(variant), cam, *PC.yard_frame(variant), flags, tree_kids=variant == "ext")  # (its group of groups is an OBJECT)


@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_the_yards_frames_on_the_per_tree_route(variant, monkeypatch):
    """tests/test_gpu_parity.py's route="per_tree": every tree through the per-tree pipeline, every query sorted"""
    monkeypatch.setenv("RPTGPU_DEEP_DEPTH", "1")
    monkeypatch.setenv("RPTGPU_SORT_RAYS", "1")
    monkeypatch.setenv("RPTGPU_SORT_MIN_RAYS", "0")
    scene, cam = PC.yard(variant)
    g = GpuScene(scene, 0)
    try:
        o, d = PC.yard_rays()
        t0, n0, ob0 = yard_hits(variant)
        t1, n1, ob1 = g.closest_hit(o, d)
        assert (ob0 == ob1).all() and same(t0, t1) and same(n0, n1)
        for flags in (0, WAVEFRONT):
            check(g, cam, *PC.yard_frame(variant), flags)
    finally:
        g.close()


# ---- 4. the cube-normal tables under two negative determinants
@pytest.mark.parametrize("bounces", [0, 3])
def test_cube_normal_tables_of_mirrored_cubes(bounces, capfd):
    scene, cam = PC.table_room()
    g = GpuScene(scene, 0)
    try:
        lines = launch_lines(g, cam, capfd)
        assert lines and all(ln.startswith("rpt_paths<KdFlat>") and FUSED in ln and TABLES in ln for ln in lines), lines
        ref, cnt = PC.oracle_frame("table", scene, cam, bounces)
        img = check(g, cam, ref, cnt, PERSISTENT, bounces)
        assert np.isfinite(img).all() and (img != 0.0).any(axis=1).mean() >= 0.5
    finally:
        g.close()


# ---- 5. live updates
@pytest.mark.parametrize("name", ["sphere", "cube"])
def test_a_lamp_moved_on_a_live_handle(name):
    """shear -> mirror -> singular -> shear by set_lights: after each step the frames and the direct bake are the oracle's
    (the model's) and a fresh handle's"""
    cam = PC.CAMERA
    g = GpuScene(PC.room_case(name, "shear")[0], 0)
    try:
        first = check(g, cam, *PC.room_frame(name, "shear"), PERSISTENT)
        for placement in ("mirror", "singular", "shear"):
            g.set_lights([0], PC.room_case(name, placement)[0].lights)
            f = fresh(name, placement)
            for flags in (PERSISTENT, WAVEFRONT):
                img = check(g, cam, *PC.room_frame(name, placement), flags)
                assert same(img, f.render_batch(cam, PC.params(flags=flags)))
            got = bake(g)
            assert same(got, direct_case(name, placement)[0]) and same(got, bake(f))
            assert same(img, first) == (placement == "shear")
    finally:
        g.close()


@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_two_objects_swap_their_placements_on_a_live_handle(variant):
    """set_objects gives objects 1 and 2 each other's placement (and place): closest hits, frames and the direct bake are
    the oracle's and a fresh handle's, and the way back restores the first frame"""
    swap = (1, 0, 2, 3)
    scene, cam = PC.yard(variant)
    swapped = PC.yard(variant, swap)[0]
    o, d = PC.yard_rays()
    pos, nrm, ids = PC.points(variant)
    g = GpuScene(scene, 0)
    f = GpuScene(swapped, 0)
    try:
        first = check(g, cam, *PC.yard_frame(variant), 0)
        g.set_objects([1, 2], swapped.objects[1:3])
        t0, n0, ob0 = O.OracleScene(swapped).closest_hit(o, d)
        for h in (g, f):
            t1, n1, ob1 = h.closest_hit(o, d)
            assert (ob0 == ob1).all() and same(t0, t1) and same(n0, n1)
        assert (ob0 != yard_hits(variant)[2]).any()
        for flags in (0, WAVEFRONT):
            img = check(g, cam, *PC.yard_frame(variant, swap), flags)
            assert same(img, f.render_batch(cam, PC.params(flags=flags)))
        assert not same(img, first)
        want = DM.direct(swapped.lights, pos, nrm, SAMPLES, PC.BAKE_SEED, closest_t(f), streams=ids, illuminate=DC.oracle_illuminate)
        got = bake(g, variant)
        assert same(got, want) and same(got, bake(f, variant)) and (want != 0.0).any()
        g.set_objects([1, 2], scene.objects[1:3])
        assert same(check(g, cam, *PC.yard_frame(variant), 0), first)
    finally:
        g.close()
        f.close()
