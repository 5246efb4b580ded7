"""The guides pass and the demodulated denoise without a GPU: the header's declarations and both libraries' exports, the ctypes struct against the header's,
argument checks that come before any HIP call, Renderer.guides' and Film.denoise's own argument checks, and the declarations in INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_guides", "pt_guides_device", "pt_guides_finish", "pt_film_denoise_albedo", "pt_film_denoise_albedo_device", "pt_test_denoise_albedo_host")
HOST_CALLS = ("ph_renderer_guides", "ph_renderer_film_denoise_albedo")


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
    assert list(H.AOV_BUFFERS) == ["depth", "position", "normal", "node", "sub", "material"], "albedo is no new name of aov"
    assert [n for n, _ in H.PtDenoiseGuides._fields_] == ["position", "normal", "node"] and C.sizeof(H.PtDenoiseParams) == 32


def test_ctypes_struct_has_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    fields = ["albedo", "position", "normal", "node"]
    lines = ['printf("size %zu\\n", sizeof(pt_guides_buffers));'] + ['printf("%s %%zu\\n", offsetof(pt_guides_buffers, %s));' % (f, f) for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(H.PtGuidesBuffers)
    assert [n for n, _ in H.PtGuidesBuffers._fields_] == fields == list(H.GUIDES_BUFFERS)
    for f in fields:
        assert int(got[f]) == getattr(H.PtGuidesBuffers, f).offset, f


def test_null_context_is_an_argument_error_before_any_hip_call(H):
    lib = H.lib()
    cam = H.PtCamera()
    albedo = np.zeros((4, 4, 3))
    b = H.PtGuidesBuffers(albedo=albedo.ctypes.data_as(H._dp))
    p = H.PtAovParams(4, 4, H.PtRect(0, 0, 3, 3), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_guides(None, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_guides_device(None, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_guides_finish(None, None) == H.ERR_ARGUMENT
    node = np.zeros((4, 4), dtype=np.int32)
    g = H.PtDenoiseGuides(None, None, node.ctypes.data)
    dp = H.PtDenoiseParams(1, 0, 0.0, 0.0, -1)
    out = np.full((4, 4, 3), 7.0)
    assert lib.pt_film_denoise_albedo(None, None, C.byref(dp), C.byref(g), albedo.ctypes.data_as(H._dp), None, out.ctypes.data_as(H._dp), None) == H.ERR_ARGUMENT
    assert lib.pt_film_denoise_albedo_device(None, None, C.byref(dp), C.byref(g), albedo.ctypes.data, None, out.ctypes.data, None, None) == H.ERR_ARGUMENT
    assert np.all(out == 7.0)


def test_renderer_guides_rejects_bad_arguments_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    cam = np.zeros(10)
    with pytest.raises(ValueError, match="depth"):
        r.guides(cam, 8, 8, want=("albedo", "depth"))
    with pytest.raises(ValueError):
        r.guides(cam, 8, 8, want=())
    with pytest.raises(ValueError, match="into"):
        r.guides(cam, 8, 8, want=("albedo",), into={"albedo": np.zeros((8, 8), dtype=np.float64)})
    with pytest.raises(ValueError, match="into"):
        r.guides(cam, 8, 8, want=("node",), into={"node": np.zeros((8, 8), dtype=np.float64)})


def test_film_denoise_rejects_a_bad_albedo_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Film):
        def __init__(self):
            self._h, self._r = C.c_void_p(), None
            self.width, self.height, self.moments = 8, 4, True

    f = NoLibrary()
    cam = np.zeros(10)
    guides = {"node": np.zeros((4, 8), dtype=np.int32), "normal": np.zeros((4, 8, 3))}
    with pytest.raises(ValueError, match="albedo"):
        f.denoise(cam, albedo=np.zeros((4, 8, 3), dtype=np.float32), guides=guides)
    with pytest.raises(ValueError, match="albedo"):
        f.denoise(cam, albedo=np.zeros((4, 8)), guides=guides)
    with pytest.raises(ValueError, match="guides"):
        f.denoise(cam, albedo=np.zeros((4, 8, 3)))
    with pytest.raises(ValueError, match="albedo"):
        f.denoise(cam, albedo=True, guides=guides)
    with pytest.raises(ValueError, match="albedo"):
        f.denoise(cam, albedo="yes")


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtGuidesBuffers\s*\{[^}]*pub albedo: \*mut f64, pub position: \*mut f64, pub normal: \*mut f64, pub node: \*mut i32,\s*\}", text)
    for name in HIP_CALLS[:5]:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_film_denoise_albedo\([^)]*host_guides: \*const PtDenoiseGuides, albedo: \*const f64,", text)
    assert re.search(r"pub fn pt_film_denoise_albedo_device\([^)]*d_guides: \*const PtDenoiseGuides, d_albedo: \*const f64,", text)
