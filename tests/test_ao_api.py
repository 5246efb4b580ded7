"""The ambient-occlusion pass without a GPU: the header's declarations and both libraries' exports, the ctypes structs against the header's, every refusal that
comes before a HIP call, Renderer.ao's and Renderer.ao_camera's own argument checks, and the declarations in INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_ao", "pt_ao_device", "pt_ao_finish", "pt_test_ao_rays_host", "pt_test_ao_tables")
HOST_CALLS = ("ph_renderer_ao", "ph_renderer_ao_camera")
PARAM_FIELDS = ["n", "samples", "pass", "seed", "first_index", "radius", "bias", "flags", "eye"]  # the header's names; ctypes says pass_index (`pass` is a keyword)
BUFFER_FIELDS = ["occluded", "valid", "bent"]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_header_declares_the_calls_and_the_libraries_export_them(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HIP_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name), name
    assert not H.missing_symbols()
    from portrayer_amd import host
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HOST_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in host.EXPORTS and hasattr(host.lib(), name), name


def test_the_additions_move_nothing_that_exists(H):
    assert H.lib().pt_abi_version() == 8
    assert list(H.RAYS_BUFFERS) == ["t", "position", "normal", "node", "sub", "material", "occluded"] and C.sizeof(H.PtRaysParams) == 16
    assert H.AO_MAX == H.RAYS_MAX // 64 == 1 << 24


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("params %zu\\n", sizeof(pt_ao_params));', 'printf("buffers %zu\\n", sizeof(pt_ao_buffers));',
             'printf("FACE_EYE %u\\n", (unsigned)PT_AO_FACE_EYE);', 'printf("MAX %llu\\n", (unsigned long long)PT_AO_MAX);']
    lines += ['printf("p.%s %%zu\\n", offsetof(pt_ao_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['printf("b.%s %%zu\\n", offsetof(pt_ao_buffers, %s));' % (f, f) for f in BUFFER_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(H.PtAoParams) and int(got["buffers"]) == C.sizeof(H.PtAoBuffers)
    assert int(got["FACE_EYE"]) == H.AO_FACE_EYE and int(got["MAX"]) == H.AO_MAX
    assert [n for n, _ in H.PtAoParams._fields_] == [f if f != "pass" else "pass_index" for f in PARAM_FIELDS]
    assert [n for n, _ in H.PtAoBuffers._fields_] == BUFFER_FIELDS == list(H.AO_BUFFERS)
    for f in PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(H.PtAoParams, f if f != "pass" else "pass_index").offset, f
    for f in BUFFER_FIELDS:
        assert int(got["b." + f]) == getattr(H.PtAoBuffers, f).offset, f


def test_null_arguments_are_argument_errors_before_any_hip_call(H):
    lib = H.lib()
    P, N, occ = np.zeros((4, 3)), np.ones((4, 3)), np.full(4, 7, dtype=np.uint32)
    p = H.PtAoParams(4, 16, 0, 0, 0, 1.0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    b = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.pt_ao(None, C.byref(p), dp(P), dp(N), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_ao_device(None, C.byref(p), P.ctypes.data, N.ctypes.data, C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_ao_finish(None, None) == H.ERR_ARGUMENT
    assert lib.pt_test_ao_tables(None, None) == H.ERR_ARGUMENT
    assert np.all(occ == 7)


def test_every_refusal_of_the_parameter_block_is_an_argument_error_without_a_context(H):
    """pt_ao's checks run in the header's order and a NULL context is the first of them, so with no GPU every call below is PT_ERR_ARGUMENT for that reason alone;
    what pins each refusal of the parameter block here is pt_test_ao_rays_host, which asks the very function pt_ao asks (tests/test_gpu_ao.py repeats them on a
    context). Nothing is written either way."""
    lib = H.lib()
    P, N = np.zeros((4, 3)), np.ones((4, 3))
    O, D, valid, occ = np.full((4, 64, 3), 7.0), np.full((4, 64, 3), 7.0), np.full(4, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ok = dict(n=4, samples=16, pass_index=0, seed=0, first_index=0, radius=1.0, bias=0.0, flags=0)
    bad = [dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=128), dict(radius=float("nan")), dict(radius=1e-5), dict(radius=0.0), dict(bias=-1.0),
           dict(bias=float("inf")), dict(flags=2), dict(flags=H.AO_FACE_EYE | 4)]
    for change in bad:
        p = H.PtAoParams(**dict(ok, **change))
        assert lib.pt_test_ao_rays_host(4, C.byref(p), dp(P), dp(N), dp(O), dp(D), valid.ctypes.data_as(H._u8p)) == H.ERR_ARGUMENT, change
        assert lib.pt_ao(None, C.byref(p), dp(P), dp(N), C.byref(H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))), None) == H.ERR_ARGUMENT, change
    p = H.PtAoParams(**dict(ok, flags=H.AO_FACE_EYE))
    p.eye[2] = float("inf")
    assert lib.pt_test_ao_rays_host(4, C.byref(p), dp(P), dp(N), dp(O), dp(D), valid.ctypes.data_as(H._u8p)) == H.ERR_ARGUMENT
    assert np.all(O == 7.0) and np.all(D == 7.0) and np.all(valid == 7) and np.all(occ == 7)
    p = H.PtAoParams(**ok)
    for args in ((None, dp(N), dp(O), dp(D), valid.ctypes.data_as(H._u8p)), (dp(P), None, dp(O), dp(D), valid.ctypes.data_as(H._u8p)), (dp(P), dp(N), None, dp(D), valid.ctypes.data_as(H._u8p)),
                 (dp(P), dp(N), dp(O), dp(D), None)):
        assert lib.pt_test_ao_rays_host(4, C.byref(p), *args) == H.ERR_ARGUMENT


def test_renderer_ao_rejects_bad_arguments_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    P, N = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="want"):
        r.ao(P, N, want=("occluded", "depth"))
    with pytest.raises(ValueError, match="want"):
        r.ao(P, N, want=())
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.ao(P, N[:7])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.ao(P.ravel(), N.ravel())
    with pytest.raises(ValueError, match="float64"):
        r.ao(P.astype(np.float32), N.astype(np.float32))
    for S in (0, 3, 128, 16.0, True, None):
        with pytest.raises(ValueError, match="samples"):
            r.ao(P, N, samples=S)
    for radius in (float("nan"), 1e-5, 0.0, -1.0, "far", None):
        with pytest.raises(ValueError, match="radius"):
            r.ao(P, N, radius=radius)
    for bias in (-1e-9, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="bias"):
            r.ao(P, N, bias=bias)
    for name in ("seed", "pass_index", "first_index"):
        for v in (-1, 1.5, True, 1 << 64):
            with pytest.raises(ValueError, match=name):
                r.ao(P, N, **{name: v})
    with pytest.raises(ValueError, match="pass_index"):
        r.ao(P, N, pass_index=1 << 32)
    for eye in ((0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
        with pytest.raises(ValueError, match="eye"):
            r.ao(P, N, eye=eye)
    with pytest.raises(ValueError, match="into"):
        r.ao(P, N, want=("occluded",), into={"occluded": np.zeros(8, dtype=np.int32)})
    with pytest.raises(ValueError, match="into"):
        r.ao(P, N, want=("bent",), into={"bent": np.zeros(8)})
    with pytest.raises(ValueError, match="into"):
        r.ao(P, N, want=("valid",), into={"valid": [0] * 8})


def test_renderer_ao_camera_rejects_bad_arguments_before_any_library_call(H):
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    cam = np.zeros(10)
    for w, h in ((0, 8), (8, 0), (8.0, 8), (True, 8), (-1, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.ao_camera(cam, w, h)
    with pytest.raises(ValueError, match="points"):
        r.ao_camera(cam, 8192, 4096)  # 2^25 pixels > PT_AO_MAX
    with pytest.raises(ValueError, match="samples"):
        r.ao_camera(cam, 8, 8, samples=5)
    with pytest.raises(ValueError, match="radius"):
        r.ao_camera(cam, 8, 8, radius=0.0)
    with pytest.raises(ValueError, match="into"):
        r.ao_camera(cam, 8, 4, want=("bent",), into={"bent": np.zeros((8, 4, 3))})
    with pytest.raises(ValueError, match="cam10"):
        r.ao_camera(np.zeros(9), 8, 8)
    with pytest.raises(ValueError, match="want"):
        r.ao_camera(cam, 8, 8, want=("visibility",))


def test_the_host_library_refuses_null_and_oversized_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    p = H.PtAoParams(4, 16, 0, 0, 0, 1.0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    occ = np.zeros(4, dtype=np.uint32)
    b = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))
    P = np.zeros((4, 3))
    assert lib.ph_renderer_ao(None, C.byref(p), P.ctypes.data_as(H._dp), P.ctypes.data_as(H._dp), C.byref(b), None) == -1
    cam = np.zeros(10)
    assert lib.ph_renderer_ao_camera(None, cam.ctypes.data_as(H._dp), 2, 2, C.byref(p), C.byref(b), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtAoParams\s*\{[^}]*pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,\s*pub radius: f64, pub bias: f64, "
                     r"pub flags: u32, pub eye: \[f64; 3\],\s*\}", text)
    assert re.search(r"pub struct PtAoBuffers\s*\{[^}]*pub occluded: \*mut u32, pub valid: \*mut u8, pub bent: \*mut f64,\s*\}", text)
    for name in HIP_CALLS[:3]:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_ao\([^)]*params: \*const PtAoParams, positions: \*const f64, normals: \*const f64, host_out: \*const PtAoBuffers,", text)
    assert re.search(r"pub const PT_AO_FACE_EYE: u32 = 1;", text)
