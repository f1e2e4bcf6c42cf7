"""The null-stream rule of the Python binding's tensor calls on a real MI355X, for the calls whose own tests have no late
producer: bake_probes, occluded, bake_ao, first_hits, hit_surface, set_mesh and set_group (trace_rays and trace_vertices
have theirs in test_gpu_trace_rays.py and test_gpu_vertices.py, whose pattern this follows).

The inputs are still being PRODUCED when the call is made: the tensors hold zeros until a copy that stands behind some
30 ms of queued kernels on the producer's stream has run.  The handle's stream is not ordered with any of torch's, so a
call that does not wait for the producer reads the zeros.  On torch's default stream (the null stream, which has no
handle to give the library: the wrapper waits) and on a stream of its own (the library waits for the handle it is
given), the result must be the host call's, bit for bit.  Tolerance 0."""
import functools

import numpy as np
import pytest

from rpt_amd import GpuScene, _abi, make_params, transform_records

import small_scenes

pytestmark = pytest.mark.gpu

N = 256
MESH, GROUP = 5, 6  # coverage's top-level Mesh and its KdTree of spheres and cubes: the smallest scene that has both


@functools.lru_cache(maxsize=None)
def coverage():
    scene, camera, _ = small_scenes.small("coverage")
    return scene, camera, make_params(32, 18, 2, 2, seed=0x5752)


@functools.lru_cache(maxsize=None)
def inputs():
    """256 rays from around the camera into the scene (half of them at the mesh), 256 points with unit normals, distances
    and stream ids that are not the indices — shared, never written to"""
    rs = np.random.RandomState(0x5752)
    o = np.array([0.5, 2.2, 7.0]) + rs.uniform(-0.2, 0.2, (N, 3))
    at = rs.uniform((-2.5, -1.0, -2.0), (2.5, 2.5, 1.5), (N, 3))
    at[::2] = np.array([0.0, 1.2, 0.5]) + rs.uniform(-0.8, 0.8, (N // 2, 3))
    d = at - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pos = rs.uniform((-2.5, -0.9, -2.0), (2.5, 3.0, 2.0), (N, 3))
    nrm = rs.standard_normal((N, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    max_t = rs.uniform(4.0, 12.0, N)
    ids = (np.arange(N, dtype=np.int32)[::-1] + 1000).copy()
    return dict(o=o, d=d, pos=pos, nrm=nrm, max_t=max_t, ids=ids)


def mesh_rows():
    """the mesh's triangles at creation, and the rows it deforms to"""
    from rpt_amd import scenes
    base = scenes.knot_mesh(24, 6)
    moved = base.copy()
    moved[:, :9] *= 1.0 + 0.2 * np.sin(3.0 * base[:, :9])
    return base, moved


def group_records():
    """the group's records at creation, and those of its children a step to the side"""
    kids = coverage()[0].objects[GROUP].shape.shape.objects
    return transform_records(kids), transform_records([k.translate((0.1, 0.2, -0.1)) for k in kids])


def frame(g):
    scene, camera, p = coverage()
    return g.render_batch(camera, p)


def set_mesh(g, rows):
    g.set_mesh(MESH, mesh_rows()[0])  # (through the host, so that a call that changed nothing cannot pass)
    g.set_mesh(MESH, rows)
    return frame(g)


def set_group(g, records):
    g.set_group(GROUP, group_records()[0])
    g.set_group(GROUP, records)
    return frame(g)


# name -> (the arrays that go in, the call on them)
CASES = {
    "bake_probes": (lambda: [inputs()[k] for k in ("pos", "nrm", "ids")],
                    lambda g, pos, nrm, ids: g.bake_probes(pos, nrm, kind=_abi.RPT_PROBE_IRRADIANCE, samples=2, max_bounces=2,
                                                           seed=11, streams=ids)),
    "occluded": (lambda: [inputs()[k] for k in ("o", "d", "max_t")], lambda g, o, d, max_t: g.occluded(o, d, max_t=max_t)),
    "bake_ao": (lambda: [inputs()[k] for k in ("pos", "nrm", "ids")],
                lambda g, pos, nrm, ids: g.bake_ao(pos, nrm, samples=2, seed=12, max_distance=3.0, streams=ids, bent_normals=True)),
    "first_hits": (lambda: [inputs()[k] for k in ("o", "d")], lambda g, o, d: g.first_hits(o, d)),
    "hit_surface": (lambda: [inputs()[k] for k in ("o", "d")], lambda g, o, d: g.hit_surface(o, d)),
    "set_mesh": (lambda: [mesh_rows()[1]], set_mesh),
    "set_group": (lambda: [group_records()[1]], set_group),
}


def bits(result):
    """a call's result as a list of numpy arrays"""
    if isinstance(result, dict):
        result = [result[k] for k in sorted(result)]
    elif not isinstance(result, (tuple, list)):
        result = [result]
    return [r if isinstance(r, np.ndarray) else r.cpu().numpy() for r in result]


def same(got, want):
    return len(got) == len(want) and all(a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_late_producer_is_waited_for(name):
    import torch
    arrays, call = CASES[name]
    arrays = arrays()
    dev = torch.device("cuda", 0)
    g = GpuScene(coverage()[0], 0)
    host = call(g, *arrays)
    want = bits(host)
    if name == "hit_surface":
        assert (host["primitive"] >= 0).any() and (host["child"] >= 0).any()  # the mesh and the group are hit
    if name in ("set_mesh", "set_group"):
        fresh = GpuScene(coverage()[0], 0)
        assert not same(want, [frame(fresh)])  # the update shows in the frame
        fresh.close()
    ready = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    assert same(bits(call(g, *ready)), want)
    ballast = torch.ones(64 << 20, dtype=torch.float32, device=dev)
    for stream in (torch.cuda.current_stream(dev), torch.cuda.Stream(dev)):
        late = [torch.zeros_like(t) for t in ready]
        stream.wait_stream(torch.cuda.current_stream(dev))  # (the zeros above are there)
        with torch.cuda.stream(stream):
            for _ in range(200):
                ballast.mul_(1.0)
            for l, t in zip(late, ready):
                l.copy_(t)
            got = bits(call(g, *late))
        assert same(got, want), "default stream" if stream.cuda_stream == 0 else "a stream of its own"
        torch.cuda.current_stream(dev).wait_stream(stream)
    g.close()
