"""The probe volume's use case on a real MI355X (include/rpt_gpu_probe_volume.h): what moves on a live handle has
no lightmap chart that stays true, and is lit by the probes.  After set_objects has moved the Cornell box's small cube, the ray
form and the views form on the SAME handle equal a fresh handle's on the updated scene in every bit, and differ from the
results before the update exactly where the cube was or is."""
import numpy as np
import pytest
import torch  # noqa: F401  before the library is loaded: a process gets ONE HIP runtime

import rpt_amd
from rpt_amd import GpuScene

import small_scenes
import test_gpu_lightmap_lookup as LK
import test_gpu_probe_volume as T

pytestmark = pytest.mark.gpu

CUBE = 6
W, H = 16, 9


def moved_scene():
    """test_gpu_first_hits' move of the small cube, with a new colour"""
    moved, _, _ = rpt_amd.scenes.cornell()
    moved.objects[CUBE] = rpt_amd.Object(rpt_amd.cube().scale((165.0, 165.0, 165.0)).rotate_y(0.4).translate((300.0, 120.0, 140.0))) \
        .material(rpt_amd.Material.diffuse(rpt_amd.hex_color(0x3366CC)))
    return moved


def test_after_set_objects_the_ray_form_and_the_views_form_are_a_fresh_handles():
    name = "cornell"
    o, d, _ = T.rays(name)
    vol, bias = T.scene_volume(name, "half"), 3.0
    binds = [LK.bindings(name, "large")[0]]
    views = LK.the_views(name)
    kw = dict(samples=2, seed=0x5056, seed_stride=1, normal_bias=bias, unbound_irradiance=T.UNBOUND)
    g = GpuScene(small_scenes.small(name)[0], 0)
    rays_before = g.lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=T.FALLBACK)
    views_before = g.render_views_probe_lit(views, W, H, binds, vol, **kw)
    moved = moved_scene()
    g.set_objects([CUBE], [moved.objects[CUBE]])
    rays_after = g.lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=T.FALLBACK)
    views_after = g.render_views_probe_lit(views, W, H, binds, vol, **kw)
    fresh = GpuScene(moved, 0)
    rays_fresh = fresh.lookup_probe_volume(o, d, vol, normal_bias=bias, fallback=T.FALLBACK)
    views_fresh = fresh.render_views_probe_lit(views, W, H, binds, vol, **kw)
    g.close()
    fresh.close()
    assert T.differing(rays_after, rays_fresh, T.RAY_NAMES) == []
    assert T.same(views_after, views_fresh)
    # the update is seen, and only at the moved object: a ray that hits the cube neither before nor after keeps its record
    cube = (rays_before["object"] == CUBE) | (rays_after["object"] == CUBE)
    assert cube.sum() >= 5 and (rays_after["object"] == CUBE).any()
    changed = (T.M.bits(rays_after["value"]) != T.M.bits(rays_before["value"])).any(axis=1)
    assert changed[cube].any()
    for k in T.RAY_NAMES:
        assert T.same(rays_after[k][~cube], rays_before[k][~cube]), k
    assert not T.same(views_after, views_before)
