"""rptgpu_trace_vertices on a handle that has been UPDATED: after set_objects, set_lights, set_mesh and set_group — one case
each of tests/update_cases.py, the fixtures of test_gpu_update_matrix.py — every channel is, bit for bit, that of a fresh
handle of the updated scene (DESIGN.md §9's contract; a NaN equals the same NaN, -0.0 differs from +0.0).  The handle is warm:
the call has run on it before the update, so its workspace, its staging array and its record ratio are the old scene's."""
import numpy as np
import pytest
import torch  # before the library is loaded: a process gets ONE HIP runtime, and torch only finds the GPU through its own

from rpt_amd import GpuScene, _abi

import update_cases as C

pytestmark = pytest.mark.gpu

# (case, the live update its first step applies)
CASES = [("objects_flat", "set_objects"), ("lights", "set_lights"), ("mesh_same_depth", "set_mesh"), ("group_per_tree", "set_group")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def differing(got, want):
    got, want = got.arrays(), want.arrays()
    return sorted(k for k in set(got) | set(want) if k not in got or k not in want or got[k].shape != want[k].shape
                  or not np.array_equal(bits(got[k]), bits(want[k])))


def vertices(h, name, **kw):
    o, d, _ = C.rays(name)
    ids = (np.arange(len(o), dtype=np.uint32) * 7 + 3)  # stream ids that are not the indices
    return h.trace_vertices(o, d, C.BOUNCES, samples=C.SPP, seed=11, sample_index_base=C.BASE, streams=ids, **kw)


@pytest.mark.parametrize("name,update", CASES, ids=[c[0] for c in CASES])
def test_an_updated_handle_gives_a_fresh_handles_vertices(name, update):
    c = C.cases()[name]
    step = c.steps[0]
    assert not step.back
    g = GpuScene(c.scene0, 0, **c.options)
    f = GpuScene(step.scene, 0, **c.options)
    try:
        warm = vertices(g, name)
        assert warm.channels == _abi.RPT_VERTEX_ALL and (warm.length >= 1).all()
        assert len(np.unique(warm.length)) >= 2 and (warm.object[:, :, 0] >= 0).mean() >= 0.10
        step.apply(g)
        got, want = vertices(g, name), vertices(f, name)
        assert differing(got, want) == [], "%s after %s: differs from a fresh handle" % (name, update)
        general = vertices(g, name, flags=_abi.RPT_FLAG_GENERAL_TRAVERSAL)
        assert differing(general, want) == [], "%s after %s under RPT_FLAG_GENERAL_TRAVERSAL" % (name, update)
        assert differing(got, warm) != [], "the update is not seen"
    finally:
        g.close()
        f.close()
