"""First-hit feature buffers without a GPU: the symbol and the struct's layout, every refusal of rptgpu_render_aov (all of
them come before any device work), no CPU fallback, and the oracle model of tests/aov_model.py against a second,
independently written fold."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rpt_amd
from rpt_amd import _abi

import aov_model as M
import small_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _abi.RPTGPU_E_INVALID_ARGUMENT


def test_symbol_and_struct_size_match_the_header(tmp_path):
    lib = _abi.load_library()
    assert hasattr(lib, "rptgpu_render_aov")
    fields = ("channels", "hits", "depth", "normal", "albedo", "position", "object")
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rpt_gpu.h"\nint main(void){printf("%zu", sizeof(RptAovBuffers));' + \
          "".join('printf(" %%zu", offsetof(RptAovBuffers, %s));' % f for f in fields) + \
          'printf(" %d\\n", RPT_AOV_DEPTH | RPT_AOV_NORMAL | RPT_AOV_ALBEDO | RPT_AOV_POSITION | RPT_AOV_OBJECT);return 0;}'
    c = tmp_path / "sz.c"
    c.write_text(src)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(_abi.RptAovBuffers) == nums[0] == 56
    assert [getattr(_abi.RptAovBuffers, f).offset for f in fields] == nums[1:-1]
    assert nums[-1] == _abi.RPT_AOV_ALL == rpt_amd.RPT_AOV_ALL
    assert (rpt_amd.RPT_AOV_DEPTH, rpt_amd.RPT_AOV_NORMAL, rpt_amd.RPT_AOV_ALBEDO, rpt_amd.RPT_AOV_POSITION,
            rpt_amd.RPT_AOV_OBJECT) == (1, 2, 4, 8, 16)


def _buffers(n, channels=_abi.RPT_AOV_ALL):
    keep = {"hits": np.full(n, 7, dtype=np.uint32), "depth": np.full(n, 7.0), "normal": np.full(3 * n, 7.0),
            "albedo": np.full(3 * n, 7.0), "position": np.full(3 * n, 7.0), "object": np.full(n, 7, dtype=np.int32)}
    b = _abi.RptAovBuffers()
    b.struct_size, b.channels = C.sizeof(_abi.RptAovBuffers), channels
    types = dict(_abi.RptAovBuffers._fields_)
    for name, a in keep.items():
        setattr(b, name, a.ctypes.data_as(types[name]))
    return b, keep


def test_every_refusal_comes_before_the_device():
    lib = _abi.load_library()
    cam = _abi.RptCamera()
    good_p = rpt_amd.make_params(8, 8, 1, 2)
    good_b, keep = _buffers(64)

    def call(p=good_p, b=good_b, camera=cam):
        rc = lib.rptgpu_render_aov(None, C.byref(camera) if camera is not None else None,
                                   C.byref(p) if p is not None else None, C.byref(b) if b is not None else None)
        return rc, lib.rptgpu_last_error_detail(None) or b""

    # a bad RptAovBuffers: refused first, whatever else is missing (no handle, no device)
    rc, why = call(b=None)
    assert rc == E and b"RptAovBuffers" in why
    for size in (0, 48, 64):
        bad, _ = _buffers(64)
        bad.struct_size = size
        rc, why = call(b=bad)
        assert rc == E and b"struct_size" in why, size
    for bit in (32, 1 << 31, 64 | 1):
        bad, _ = _buffers(64, bit)
        rc, why = call(b=bad)
        assert rc == E and b"channels" in why, bit
    bad, _ = _buffers(64)
    bad.hits = None
    rc, why = call(b=bad)
    assert rc == E and b"hits" in why
    for bit, name in ((1, "depth"), (2, "normal"), (4, "albedo"), (8, "position"), (16, "object")):
        bad, _ = _buffers(64)
        setattr(bad, name, None)
        rc, why = call(b=bad)
        assert rc == E and name.encode() in why, name
        bad.channels = _abi.RPT_AOV_ALL & ~bit  # not named: its pointer is not looked at; the next check speaks
        rc, why = call(b=bad)
        assert rc == E and name.encode() not in why and b"handle" in why, name
    # params
    rc, why = call(p=None)
    assert rc == E and b"params" in why
    for field, value, word in (("iterations", 0, b"iterations"), ("width", 0, b"width * height"), ("height", 0, b"width * height"),
                               ("precision_mode", 1, b"precision_mode")):
        bad = rpt_amd.make_params(8, 8, 1, 2)
        setattr(bad, field, value)
        rc, why = call(p=bad)
        assert rc == E and word in why, (field, why)
    rc, why = call(camera=None)
    assert rc == E and b"camera" in why
    rc, why = call()
    assert rc == E and b"handle" in why
    # nothing was written by any of them
    assert all((a == 7).all() for a in keep.values())


def test_no_cpu_fallback(gpu_available):
    """With valid arguments and no GPU there is no handle to be had: RPTGPU_E_NO_DEVICE, never buffers from the host."""
    scene, camera, _ = rpt_amd.scenes.sphere_scene()
    r = rpt_amd.Renderer(scene, camera).width(8).height(8).num_samples(2)
    if gpu_available:
        out = r.render_aovs()
        assert out["hits"].shape == (8, 8) and out["hits"].max() <= 2
        return
    with pytest.raises(rpt_amd.RptGpuError) as e:
        r.render_aovs()
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE
    with pytest.raises(rpt_amd.RptGpuError) as e:
        rpt_amd.GpuScene(scene).render_aov(camera, rpt_amd.make_params(8, 8, 0, 2))
    assert e.value.code == _abi.RPTGPU_E_NO_DEVICE


def _second_fold(scene, camera, params, oracle):
    """The contract written a second time, on Python floats and one ray at a time: per pixel and sample its own
    oracle_camera_ray and its own oracle_closest_hit call, plain scalar additions in sample order."""
    osc = oracle.OracleScene(scene)
    own = M.owned(params)
    h, w = params.height, params.width
    out = {"hits": np.zeros((h, w), dtype=np.uint32), "depth": np.zeros((h, w)), "normal": np.zeros((h, w, 3)),
           "albedo": np.zeros((h, w, 3)), "position": np.zeros((h, w, 3)), "object": np.full((h, w), -1, dtype=np.int32)}
    for y in range(h):
        for x in range(w):
            if not own[y, x]:
                continue
            hits, depth, nrm, alb, pos = 0, 0.0, [0.0] * 3, [0.0] * 3, [0.0] * 3
            for s in range(params.iterations):
                o, d = oracle.camera_ray(camera, params, x, y, params.sample_index_base + s)
                t, n, ob = osc.closest_hit(o[None, :], d[None, :])
                if s == 0:
                    out["object"][y, x] = ob[0]
                if ob[0] < 0:
                    continue
                col = scene.objects[int(ob[0])]._material.color
                tt = float(t[0])
                hits += 1
                depth += tt
                for c in range(3):
                    nrm[c] += float(n[0, c])
                    alb[c] += float(col[c])
                    prod = tt * float(d[c])
                    pos[c] += float(o[c]) + prod
            out["hits"][y, x], out["depth"][y, x] = hits, depth
            out["normal"][y, x], out["albedo"][y, x], out["position"][y, x] = nrm, alb, pos
    return out


@pytest.mark.parametrize("name,size,part", [("sphere", (24, 14), (0, 1)), ("coverage", (20, 12), (1, 3))])
def test_the_model_equals_an_independent_fold(name, size, part, oracle):
    scene, camera, p0 = small_scenes.small(name)
    p = rpt_amd.make_params(size[0], size[1], 0, 3, seed=p0.seed, sample_index_base=5, tile=(8, 4), part=part,
                            exposure_value=p0.exposure_value)
    want = _second_fold(scene, camera, p, oracle)
    got = M.full_frame(M.expected(scene, camera, p), p)
    assert M.mismatches(got, want) == []
    own = M.owned(p)
    assert got["hits"][own].max() == 3 and (got["hits"][~own] == 0).all() and (got["object"][~own] == -1).all()
    assert 0 < (got["hits"] > 0).sum()
    assert (got["depth"][got["hits"] == 0] == 0).all()
