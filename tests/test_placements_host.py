"""Sampled shapes under sheared, mirrored, matrix and singular placements, without a GPU: the oracle's Transformed::sample
against a numpy restatement of shape.rs:139-150 over the host mirror's five fields; closed forms that need no oracle (a
uniformly sampled flat face has pdf 1 / (world area)); the sign of the pdf under a negative determinant and its loss under
a singular one; and the caps that keep tests/test_gpu_placements.py from passing on empty signals — held by the reference
alone, here."""
import numpy as np
import pytest

from oracle import oracle_ffi as O
from rpt_amd import cube

import direct_cases as DC
import direct_model as DM
import placement_cases as PC

EPS = np.finfo(np.float64).eps
N_TARGETS = 40
OPEN = ("shear", "mirror", "matrix")  # the placements of the closed forms


def targets(seed):
    """points of the room, around and below the lamp"""
    rs = np.random.RandomState(seed)
    return rs.uniform((20.0, 10.0, 20.0), (540.0, 540.0, 540.0), (N_TARGETS, 3))


def draws(i):
    return dict(seed=PC.SEED, pixel=7 + 13 * i, sample=i % 5, draw=2 * (i % 3))


def mat(m, n):
    return np.array(m, dtype=np.float64).reshape(n, n).T  # column-major -> [row][col]


def mul(m, v):
    """m * v column by column, as glm does: no library product, no fused operation"""
    acc = m[:, 0] * v[0]
    for k in range(1, len(v)):
        acc = acc + m[:, k] * v[k]
    return acc


def restated(placed, target, kw):
    """shape.rs:139-150 over the host mirror's fields and the oracle's sample of the inner shape on the same draws
    -> (v, n, p, the inner shape's v, n, p)"""
    fwd, inv = mat(placed.transform_m, 4), mat(placed.inverse_transform, 4)
    lin, nt = mat(placed.linear, 3), mat(placed.normal_transform, 3)
    with np.errstate(all="ignore"):
        local = mul(inv, np.append(target, 1.0))[:3]
        v, n, p, _ = O.shape_sample(placed.shape, local, **kw)
        new_normal = DM.normalize(mul(nt, n))
        height = DM.dot(mul(lin, n), new_normal)
        base = placed.scale_det / height
        return mul(fwd, np.append(v, 1.0))[:3], new_normal, p / base, v, n, p


def ulps(a, b):
    """|a - b| in ulps of the larger magnitude of the two (vectors: of their largest component); NaN where both are NaN
    counts as 0, where one is as inf"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    both = np.isnan(a) & np.isnan(b)
    if (np.isnan(a) != np.isnan(b)).any():
        return float("inf")
    if both.all():
        return 0.0
    a, b = a[~both], b[~both]
    if (np.isinf(a) | np.isinf(b)).any():
        return 0.0 if (a == b).all() else float("inf")
    scale = max(np.abs(a).max(), np.abs(b).max())
    return float(np.abs(a - b).max() / np.spacing(scale)) if scale > 0.0 else 0.0


@pytest.mark.parametrize("name", PC.LAMPS)
def test_the_oracles_sample_is_the_restatement_of_the_reference(name):
    """Tolerance 16 ulp: the chain is two 3 x 3 products, a normalisation, a dot product and two divisions, under twenty
    roundings (a local target that differs in its last bit moves a sphere's sample by as little)."""
    worst = (0.0, ("", "", 0))
    for placement in PC.PLACEMENTS:
        placed = PC.room_lamp(name, placement)
        for i, target in enumerate(targets(len(name) + len(placement))):
            kw = draws(i)
            v, n, p, _ = O.shape_sample(placed, target, **kw)
            rv, rn, rp = restated(placed, target, kw)[:3]
            for what, a, b in (("v", v, rv), ("n", n, rn), ("p", p, rp)):
                u = ulps(a, b)
                worst = max(worst, (u, (placement, what, i)))
                assert u <= 16.0, (name, placement, what, i, a, b)
    print("%s: worst deviation %.2f ulp = %.2e relative at %s" % (name, worst[0], worst[0] * EPS, worst[1]))


@pytest.mark.parametrize("name", PC.LAMPS)
@pytest.mark.parametrize("placement", PC.PLACEMENTS)
def test_the_sign_of_the_pdf_is_the_determinants(name, placement):
    """p < 0 for every sample of a shape whose own pdf is positive under `mirror`, `matrix` and `bottom_row`; a group's
    children stand under a second negative determinant, so its leaves have the opposite sign (placement_cases.leaf_sign);
    under `singular` no pdf is finite"""
    placed = PC.room_lamp(name, placement)
    want = PC.leaf_sign(name, placement)
    assert np.sign(placed.scale_det) == {"shear": 1, "singular": 0}.get(placement, -1)
    for i, target in enumerate(targets(3)):
        p = O.shape_sample(placed, target, **draws(i))[2]
        assert (not np.isfinite(p)) if want == 0 else (np.isfinite(p) and np.sign(p) == want), (name, placement, i, p)


def triangle_of(rows, local):
    """which triangle of a flat mesh in the plane y = 0 holds the local point"""
    for k, row in enumerate(rows):
        a, b, c = row[0:3], row[3:6], row[6:9]
        m = np.array([[b[0] - a[0], c[0] - a[0]], [b[2] - a[2], c[2] - a[2]]])
        u, v = np.linalg.solve(m, [local[0] - a[0], local[2] - a[2]])
        if u >= -1e-9 and v >= -1e-9 and u + v <= 1.0 + 1e-9:
            return k
    raise AssertionError(local)


@pytest.mark.parametrize("placement", OPEN)
@pytest.mark.parametrize("name", ["quad", "pentagon"])
def test_a_flat_lamps_pdf_is_one_over_its_world_area(name, placement):
    """|p| * (world area of the sampled triangle) * num_triangles == 1 to 8 ulp, the area from cross(M e1, M e2): no
    inverse, no normal transform and no determinant on this side"""
    placed = PC.room_lamp(name, placement)
    rows = placed.shape.triangles
    lin = mat(placed.linear, 3)
    seen, worst = set(), 0.0
    for i, target in enumerate(targets(5)):
        kw = draws(i)
        p = O.shape_sample(placed, target, **kw)[2]
        local = O.shape_sample(placed.shape, target, **kw)[0]  # (a mesh's sample does not read its target)
        k = triangle_of(rows, local)
        seen.add(k)
        e1, e2 = rows[k][3:6] - rows[k][0:3], rows[k][6:9] - rows[k][0:3]
        area = 0.5 * np.linalg.norm(np.cross(mul(lin, e1), mul(lin, e2)))
        worst = max(worst, ulps(abs(p) * area * len(rows), 1.0))
    assert len(seen) == len(rows)  # every triangle was drawn
    assert worst <= 8.0, worst


@pytest.mark.parametrize("placement", OPEN)
def test_a_cube_lamps_pdf_is_one_over_six_world_faces(placement):
    """|p| * 6 * (world area of the sampled face) == 1 to 8 ulp"""
    placed = PC.room_lamp("cube", placement)
    lin = mat(placed.linear, 3)
    seen, worst = set(), 0.0
    for i, target in enumerate(targets(6)):
        kw = draws(i)
        p = O.shape_sample(placed, target, **kw)[2]
        n = O.shape_sample(cube(), target, **kw)[1]
        axis = int(np.flatnonzero(n != 0.0)[0])
        seen.add((axis, float(n[axis])))
        ea, eb = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]
        area = np.linalg.norm(np.cross(mul(lin, ea), mul(lin, eb)))
        worst = max(worst, ulps(abs(p) * 6.0 * area, 1.0))
    assert len(seen) >= 5
    assert worst <= 8.0, worst


# ---- the caps: what the GPU tests compare is there, by the reference alone
def fractions(img):
    return ((img != 0.0).any(axis=1).mean(), (img < 0.0).any(axis=1).mean(), (~np.isfinite(img)).any(axis=1).mean())


@pytest.mark.parametrize("placement", PC.PLACEMENTS)
@pytest.mark.parametrize("name", PC.LAMPS)
def test_every_rooms_frame_shows_its_lamp(name, placement):
    nonzero, negative, nonfinite = fractions(PC.room_frame(name, placement)[0])
    assert nonzero >= 0.5
    sign = PC.leaf_sign(name, placement)
    if sign < 0:
        assert negative >= 0.5
    elif sign > 0:
        assert negative == 0.0 and nonfinite == 0.0
    else:
        assert nonfinite >= 0.5


def test_the_table_rooms_frames_are_lit():
    for bounces in (0, 3):
        img = PC.oracle_frame("table", *PC.table_room(), bounces=bounces)[0]
        assert fractions(img)[0] >= 0.5 and np.isfinite(img).all()


@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_the_yards_rays_hit_every_placed_object_and_miss(variant):
    scene = PC.yard(variant)[0]
    o, d = PC.yard_rays()
    t, nrm, obj = O.OracleScene(scene).closest_hit(o, d)
    placed = range(1, len(scene.objects) - 1)  # between the plane and the singular cube
    assert len(placed) == 4
    for k in placed:
        assert (obj == k).mean() >= 0.02, (k, int((obj == k).sum()))
    assert (obj < 0).mean() >= 0.10
    # glm::inverse of the singular cube's placement is zeros: its local ray is 0 + t * 0, and nothing ever hits it
    assert not (obj == len(scene.objects) - 1).any()
    assert fractions(PC.yard_frame(variant)[0])[0] >= 0.5


def lit_points(lights, key, closest):
    pos, nrm, ids = PC.points(key)
    out = DM.direct(lights, pos, nrm, 33, PC.BAKE_SEED, closest, streams=ids, illuminate=DC.oracle_illuminate)
    return out, (out != 0.0).any(axis=1)


@pytest.mark.parametrize("name", PC.LAMPS)
def test_the_rooms_bake_points_show_both_outcomes(name):
    """of the 16 points at least 4 receive direct light and at least 2 none, under every placement but one: a sphere under
    `singular` is sampled at a NaN point (its local target is 0, normalize(0) = NaN), wi is NaN, and rptgpu_bake_direct
    adds a light only where wi . n > 0 — that bake is +0 everywhere BY ITS DEFINITION, wherever the lamp or the points are"""
    oc = O.OracleScene(PC.room_case("sphere", "shear")[0])  # (the rooms share their objects: the lamp is none)
    closest = lambda o, d: oc.closest_hit(o, d)[0]
    for placement in PC.PLACEMENTS:
        out, lit = lit_points(PC.room_case(name, placement)[0].lights, "room", closest)
        if (name, placement) == ("sphere", "singular"):
            assert (out == 0.0).all() and not np.signbit(out).any()
            continue
        assert lit.sum() >= 4 and (~lit).sum() >= 2, (placement, lit)
        sign = PC.leaf_sign(name, placement)
        assert (np.isnan(out[lit]).any(axis=1).all() if sign == 0 else (np.sign(out[lit]) == sign).all()), (placement, out)


@pytest.mark.parametrize("variant", PC.YARD_VARIANTS)
def test_the_yards_bake_points_show_both_outcomes(variant):
    scene = PC.yard(variant)[0]
    oc = O.OracleScene(scene)
    out, lit = lit_points(scene.lights, variant, lambda o, d: oc.closest_hit(o, d)[0])
    assert lit.sum() >= 4 and (~lit).sum() >= 2, lit
