"""What tests/test_gpu_routes_matrix.py relies on, held true without a GPU: by the oracle and by the library's own flattener
and scene planner (rpt_amd/csrc/host_scene.cpp, scene_plan.h through tests/cpp/routes_host.cpp) alone.  A scene that stops
exercising the route it is in the matrix for fails here, not silently there.

  camera rays   at least 5 % of the 777 camera rays of sample 0 end on the objects the scene is there for (fractal_spheres:
                on each of its six objects);
  loose rays    at least 10 % of the 600 hit something and at least 10 % miss (tests/test_gpu_update_matrix.py's bar);
  frames        every oracle frame a device result is compared with is finite and not black;
  paths         at least one path of the frame has three or more vertices;
  route, build  the planner's RPT_TRACE_* kind of every counted object, and whether the scene takes the ext build
                (RptStats can tell neither rpt_nest_trace from rpt_tree_generic nor one build from the other).
The measured shares are printed (-rP)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_model
import routes_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cases_are_the_ones_named():
    assert RC.SCENES == ("monomial", "fractal_spheres", "fractal_teapots", "nested_groups", "deep_nest")
    assert RC.W * RC.H > 3 * 256 and (RC.W * RC.H) % 256 != 0 and RC.N_RAYS > 2 * 256 and RC.N_RAYS % 256 == 88
    assert (RC.N_POINTS * RC.PROBE_SAMPLES) % 256 != 0 and RC.N_POINTS % int(RC.PIECES["probes"][1]) != 0
    assert RC.W * RC.H % int(RC.PIECES["views"][1]) != 0  # a piece ends inside a view
    for name in RC.SCENES:
        o, d = RC.rays(name)
        unit = abs((d * d).sum(axis=1) - 1.0) <= 1e-6  # no unit vectors but monomial's eight vertical rays
        assert o.shape == d.shape == (RC.N_RAYS, 3) and unit.sum() == (8 if name == "monomial" else 0)
        lens, ortho, pano = RC.views(name)
        assert lens.aperture > 0.0 and RC.scene(name)[1].aperture == 0.0
        assert sorted(v.projection for v in RC.views(name)[1:]) == [1, 2] and RC.scene(name)[2] >= 3


@pytest.mark.parametrize("name", RC.SCENES)
def test_the_oracle_alone_meets_the_floors(name):
    m = RC.measured(name)
    said = RC.said(name)
    print(said)
    on = [m["camera"].get(k, 0.0) for k in RC.COUNTED[name]]
    if name == "fractal_spheres":
        assert min(on) >= RC.SHARE, said
    else:
        assert sum(on) >= RC.SHARE, said
    assert m["hit"] >= 0.10 and m["miss"] >= 0.10, said
    assert m["long"] >= 1, said
    for what, frame in RC.oracle_frames(name).items():
        assert frame.shape == (RC.W * RC.H, 3) and np.isfinite(frame).all() and (frame != 0.0).any(), (name, what)


@pytest.mark.parametrize("name", RC.BUFFERED)
def test_the_adaptive_round_retires_some_pixels_and_keeps_others(name):
    """the device Buffer's one adaptive round stands on two plain batches, so its rule first speaks at n = 3: on the oracle's
    batches, under the GPU test's tolerance, it must leave a mix for the active count to mean something"""
    frames = [RC.view_frame(name, RC.SEEDS[0], RC.BASE + b * RC.SPP) for b in range(RC.BATCHES)]
    active = adaptive_model.run(frames, 3, 0.0, RC.ADAPTIVE_REL_TOL)["active"]
    print("%s: %d of %d pixels stay active" % (name, active[-1], RC.W * RC.H))
    assert active[:2] == [RC.W * RC.H] * 2 and 0 < active[-1] < RC.W * RC.H, active


@pytest.fixture(scope="module")
def routes(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("routes") / "libroutes_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "routes_host.cpp"),
                           os.path.join(ROOT, "rpt_amd", "csrc", "host_scene.cpp"), "-o", lib, "-lpthread"])
    L = C.CDLL(lib)
    L.routes_of.restype = C.c_int
    L.routes_of.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]

    def of(name):
        """-> ({the scene line's fields}, [{an object line's fields}])"""
        desc, keep = RC.scene(name)[0].lower()  # (as GpuScene hands the scene to rptgpu_scene_create)
        text = C.create_string_buffer(1 << 16)
        rc = L.routes_of(C.byref(desc), text, len(text))
        lines = text.value.decode().splitlines()
        print("%s:\n  %s" % (name, "\n  ".join(lines)))
        assert rc == 0 and lines[0].startswith("scene rc 0 "), lines[:1]

        def fields(line):  # "scene <name value>..." or "object <i> <name value>...": -> {name: value}
            words = line.split()
            words = words[1:] if words[0] == "scene" else words
            return dict(zip(words[0::2], (int(x) for x in words[1::2])))

        return fields(lines[0]), [fields(line) for line in lines[1:]]

    return of


@pytest.mark.parametrize("name", RC.SCENES)
def test_the_planner_gives_the_routes_and_the_build_the_matrix_says(routes, name):
    sc, objects = routes(name)
    assert sc["objects"] == len(objects) == len(RC.scene(name)[0].objects)
    assert bool(sc["ext"]) == RC.EXT[name]
    counted = [objects[k] for k in RC.COUNTED[name]]
    if name == "monomial":  # no tree anywhere: nothing for a per-tree kernel, nothing to re-order
        assert all(o["shape"] not in (RC.SHAPE_MESH, RC.SHAPE_GROUP) for o in objects) and not sc["has_deep"] and not sc["tree_kids"]
        assert all(o["shape"] == RC.SHAPE_MONOMIAL for o in counted)
        return
    groups = [o for o in counted if o["shape"] == RC.SHAPE_GROUP]
    assert len(groups) == len(counted) - (name == "fractal_spheres")  # (its sixth object is the wall)
    assert all(o["trace"] == RC.KINDS[name] for o in groups), groups
    if name == "fractal_spheres":  # walked inside rpt_extend / rpt_shadow_rays, the paths re-ordered per depth
        assert not sc["has_deep"] and not sc["tree_kids"] and sc["path_reorder"] and not sc["all_flat"]
        assert all(o["deep"] == 0 and o["kids"] == 0 for o in groups) and max(o["depth"] for o in groups) >= 3
        return
    assert sc["has_deep"] and sc["tree_kids"] and not sc["path_reorder"]  # the per-tree pipeline only
    assert all(o["deep"] != 0 for o in groups)
    if name == "fractal_teapots":  # mesh children, no group below a group: one loop over two regular levels
        assert all(o["kids"] == 1 and not o["generic_only"] for o in groups) and not sc["gen_all"]
    else:  # a group below a group: only rpt_tree_generic walks it
        assert all(o["kids"] & 2 and o["generic_only"] for o in groups) and sc["gen_all"]
