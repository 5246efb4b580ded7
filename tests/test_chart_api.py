"""The chart pass without a GPU: the header's declarations and both libraries' exports, the ctypes structs against the header's, every refusal that comes
before a HIP call and their order in the source, Renderer.chart's, ao_chart's and gather_chart's own argument checks, the per-vertex to per-corner expansion of
a UV set against Scene.export(), and the declarations in INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_chart_triangles", "pt_chart", "pt_chart_device", "pt_test_chart_host")
HOST_CALLS = ("ph_renderer_chart_triangles", "ph_renderer_chart_mesh", "ph_renderer_chart", "ph_renderer_ao_chart", "ph_renderer_gather_chart")
PARAM_FIELDS = ["node", "width", "height", "flags"]
BUFFER_FIELDS = ["position", "normal", "tri", "covered"]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_header_declares_the_calls_and_the_libraries_export_them(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HIP_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name), name
    assert re.search(r"#define PT_CHART_FLIP_NORMAL 1u", text) and H.CHART_FLIP_NORMAL == 1
    assert not H.missing_symbols()
    from portrayer_amd import host
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HOST_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in host.EXPORTS and hasattr(host.lib(), name), name


def test_the_additions_move_nothing_that_exists(H):
    assert H.lib().pt_abi_version() == 8
    assert C.sizeof(H.PtAoParams) == 80 and C.sizeof(H.PtGatherParams) == 72 and H.AO_MAX == 1 << 24


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("params %zu\\n", sizeof(pt_chart_params));', 'printf("buffers %zu\\n", sizeof(pt_chart_buffers));']
    lines += ['printf("p.%s %%zu\\n", offsetof(pt_chart_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['printf("b.%s %%zu\\n", offsetof(pt_chart_buffers, %s));' % (f, f) for f in BUFFER_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(H.PtChartParams) == 16 and int(got["buffers"]) == C.sizeof(H.PtChartBuffers) == 32
    assert [n for n, _ in H.PtChartParams._fields_] == PARAM_FIELDS
    assert [n for n, _ in H.PtChartBuffers._fields_] == BUFFER_FIELDS == list(H.CHART_BUFFERS)
    for f in PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(H.PtChartParams, f).offset, f
    for f in BUFFER_FIELDS:
        assert int(got["b." + f]) == getattr(H.PtChartBuffers, f).offset, f


def test_every_refusal_before_a_hip_call_is_an_argument_error_and_writes_nothing(H):
    """A NULL context is the first check, so with no GPU every call below is PT_ERR_ARGUMENT; the refusals of a live context are repeated where their own words
    can be read by tests/test_gpu_chart.py."""
    lib = H.lib()
    uv = np.zeros((1, 6))
    tri = np.full((2, 2), 7, dtype=np.int32)
    b = H.PtChartBuffers(tri=tri.ctypes.data_as(H._ip))
    p = H.PtChartParams(0, 2, 2, 0)
    n = C.c_uint64(7)
    assert lib.pt_chart(None, C.byref(p), uv.ctypes.data_as(H._dp), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_chart_device(None, C.byref(p), uv.ctypes.data, C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_chart_triangles(None, 0, C.byref(n)) == H.ERR_ARGUMENT and n.value == 7
    assert np.all(tri == 7)


def test_the_refusals_stand_in_the_source_in_the_headers_order_before_the_first_hip_call():
    api = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_api.hip")).read()
    start = api.index("static int pt_chart_check(")
    check = api[start:api.index("\n}\n", start)]
    start = api.index("static int pt_chart_node_check(")
    node_check = api[start:api.index("\n}\n", start)]
    for text in (check, node_check):
        assert "hip" not in text.replace("hip_stream", "") and "PT_HIP" not in text
    order = ["NULL context, params or buffers", "no output buffer asked for", "unknown flags", "width and height must be positive", "more than PT_AO_MAX texels",
             "PT_ERR_NO_SCENE", "pt_chart_node_check(", "uv is NULL", "c->aov.pass.pending"]
    at = [check.index(w) for w in order]
    assert at == sorted(at)
    assert node_check.index("flattened nodes") < node_check.index("is no mesh")
    for entry in ('extern "C" int pt_chart(', 'extern "C" int pt_chart_device('):
        s = api.index(entry)
        body = api[s:api.index("\n}\n", s)]
        assert body.index("pt_chart_check(") < body.index("PT_HIP(")
    s = api.index('extern "C" int pt_chart_device(')
    body = api[s:api.index("\n}\n", s)]
    assert body.count("pt_check_device_pointer(") == 5 and body.rindex("pt_check_device_pointer(") < body.index("pt_chart_common("), "every caller pointer, before anything is queued"
    s = api.index('extern "C" int pt_chart_triangles(')
    body = api[s:api.index("\n}\n", s)]
    assert "PT_HIP" not in body and "PT_ERR_NO_SCENE" in body
    # the words of the header's list
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    sec = header[header.index("/* ---- Chart:"):header.index("#define PT_CHART_FLIP_NORMAL")]
    assert re.search(r"Errors, before the first HIP call and in this order: PT_ERR_ARGUMENT \(a NULL context / params / buffers; no buffer asked for; unknown flags; width or height\s+\*?\s*zero", sec)


class _NoDevice:
    """Renderer.chart's checks on a renderer that has no library behind it: the node's mesh is given, any library call would fail on the null handle."""

    def __new__(cls, n_verts=5, n_tris=3):
        from portrayer_amd import host

        class NoLibrary(host.Renderer):
            def __init__(self):
                self._h = C.c_void_p()
                self.scene = None
                self._device = 0

            def _chart_node(self, node):
                if isinstance(node, bool) or not isinstance(node, (int, np.integer)) or not 0 <= int(node) < 2:
                    raise ValueError("node must index the flattened nodes")
                return int(node), n_verts, n_tris, np.array([[0, 1, 2], [2, 1, 3], [4, 3, 1]], dtype=np.uint32)[:n_tris]
        return NoLibrary()


def test_renderer_chart_rejects_bad_arguments_before_any_library_call():
    r = _NoDevice()
    uv = np.zeros((3, 6))
    for w, h in ((0, 8), (8, 0), (8.0, 8), (True, 8), (-1, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.chart(0, w, h, uv)
    with pytest.raises(ValueError, match="texels"):
        r.chart(0, 8192, 4096, uv)  # 2^25 > PT_AO_MAX
    for node in (-1, 2, 1.0, True, None):
        with pytest.raises(ValueError, match="node"):
            r.chart(node, 8, 8, uv)
    for want in ((), ("position", "depth"), ("owner",)):
        with pytest.raises(ValueError, match="want"):
            r.chart(0, 8, 8, uv, want=want)
    with pytest.raises(ValueError, match="flip_normal"):
        r.chart(0, 8, 8, uv, flip_normal=1)
    for bad in (np.zeros((4, 6)), np.zeros((3, 2, 3)), np.zeros((3, 5)), np.zeros(18), np.zeros((4, 2)), np.zeros((6, 2))):
        with pytest.raises(ValueError, match="uv must be"):
            r.chart(0, 8, 8, bad)
    with pytest.raises(ValueError, match="float64"):
        r.chart(0, 8, 8, uv.astype(np.float32))
    with pytest.raises(ValueError, match="into"):
        r.chart(0, 8, 4, uv, want=("tri",), into={"tri": np.zeros((8, 4), dtype=np.int32)})
    with pytest.raises(ValueError, match="into"):
        r.chart(0, 8, 4, uv, want=("tri",), into={"tri": np.zeros((4, 8), dtype=np.int64)})
    with pytest.raises(ValueError, match="into"):
        r.chart(0, 8, 4, uv, want=("position",), into={"position": np.zeros((4, 8))})


def test_renderer_ao_chart_and_gather_chart_reject_bad_arguments_before_any_library_call():
    r = _NoDevice()
    uv = np.zeros((3, 3, 2))
    with pytest.raises(ValueError, match="width|height"):
        r.ao_chart(0, 0, 8, uv)
    with pytest.raises(ValueError, match="samples"):
        r.ao_chart(0, 8, 8, uv, samples=3)
    with pytest.raises(ValueError, match="radius"):
        r.ao_chart(0, 8, 8, uv, radius=0.0)
    with pytest.raises(ValueError, match="uv must be"):
        r.ao_chart(0, 8, 8, np.zeros((2, 6)))
    with pytest.raises(ValueError, match="want"):
        r.ao_chart(0, 8, 8, uv, want=("visibility",))
    with pytest.raises(ValueError, match="node"):
        r.gather_chart(5, 8, 8, uv=uv)
    with pytest.raises(ValueError, match="background"):
        r.gather_chart(0, 8, 8, background=(1.0,), uv=uv)
    with pytest.raises(ValueError, match="samples"):
        r.gather_chart(0, 8, 8, uv=uv, samples=128)
    with pytest.raises(ValueError, match="into"):
        r.gather_chart(0, 8, 4, uv=uv, want=("sum",), into={"sum": np.zeros((8, 4, 3))})
    with pytest.raises(TypeError):
        r.gather_chart(0, 8, 8, uv=uv, radius=1.0)


def test_a_per_vertex_uv_set_is_expanded_through_the_meshes_indices():
    """(n_verts, 2) becomes (T, 6) by the mesh's indices; the indices ph_renderer_chart_mesh gives are Scene.export()'s for that mesh (checked on the GPU, where
    a renderer exists, by tests/test_gpu_chart.py) - here the expansion itself, and the two per-corner shapes"""
    r = _NoDevice()
    per_vertex = np.arange(10, dtype=np.float64).reshape(5, 2) / 16.0
    idx = np.array([[0, 1, 2], [2, 1, 3], [4, 3, 1]])
    p, got = r._chart_params(1, 8, 4, per_vertex, False)
    assert (p.node, p.width, p.height, p.flags) == (1, 8, 4, 0)
    assert got.shape == (3, 6) and got.flags.c_contiguous and np.array_equal(got.reshape(3, 3, 2), per_vertex[idx])
    corner = np.random.default_rng(1).uniform(size=(3, 3, 2))
    assert np.array_equal(r._chart_params(0, 8, 4, corner, True)[1], corner.reshape(3, 6)) and r._chart_params(0, 8, 4, corner, True)[0].flags == 1
    assert np.array_equal(r._chart_params(0, 8, 4, corner.reshape(3, 6), False)[1], corner.reshape(3, 6))
    assert r._chart_params(0, 8, 4, None, False)[1] is None


def test_the_host_library_refuses_null_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    cp = H.PtChartParams(0, 2, 2, 0)
    tri = np.zeros((2, 2), dtype=np.int32)
    cb = H.PtChartBuffers(tri=tri.ctypes.data_as(H._ip))
    ap = H.PtAoParams(4, 16, 0, 0, 0, 1.0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    occ = np.zeros(4, dtype=np.uint32)
    ab = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))
    gp = H.PtGatherParams(4, 16, 0, 0, 0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    total, bg = np.zeros((4, 3)), np.zeros(3)
    gb = H.PtGatherBuffers(sum=total.ctypes.data_as(H._dp))
    counts = np.zeros(2, dtype=np.uint64)
    assert lib.ph_renderer_chart(None, C.byref(cp), None, C.byref(cb), None) == -1
    assert lib.ph_renderer_chart_triangles(None, 0, counts.ctypes.data_as(H._u64p)) == -1
    assert lib.ph_renderer_chart_mesh(None, 0, counts.ctypes.data_as(H._u64p), 0, None) == -1
    assert lib.ph_renderer_ao_chart(None, C.byref(cp), None, C.byref(ap), C.byref(ab), None) == -1
    assert lib.ph_renderer_gather_chart(None, C.byref(cp), None, C.byref(gp), bg.ctypes.data_as(H._dp), C.byref(gb), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtChartParams \{ pub node: u32, pub width: u32, pub height: u32, pub flags: u32 \}", text)
    assert re.search(r"pub struct PtChartBuffers\s*\{[^}]*pub position: \*mut f64, pub normal: \*mut f64, pub tri: \*mut i32, pub covered: \*mut u8,\s*\}", text)
    assert re.search(r"pub const PT_CHART_FLIP_NORMAL: u32 = 1;", text)
    for name in HIP_CALLS[:3]:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_chart\(ctx: \*mut PtContext, params: \*const PtChartParams, uv: \*const f64, host_out: \*const PtChartBuffers, kernel_ms: \*mut f64\)", text)
