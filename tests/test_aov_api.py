"""The primary-visibility pass without a GPU: argument checks that come before any HIP call, the ctypes structs against the header's, and
Renderer.aov's own argument check."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_null_context_is_an_argument_error_before_any_hip_call(H):
    lib = H.lib()
    cam = H.PtCamera()
    depth = np.zeros((4, 4))
    b = H.PtAovBuffers(depth=depth.ctypes.data_as(H._dp))
    p = H.PtAovParams(4, 4, H.PtRect(0, 0, 3, 3), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_aov(None, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_aov_device(None, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_aov_finish(None, None) == H.ERR_ARGUMENT
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    fields = {"pt_aov_params": ["width", "height", "slice", "offset"], "pt_aov_buffers": ["depth", "position", "normal", "node", "sub", "material"]}
    lines = []
    for st, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in (("pt_aov_params", H.PtAovParams), ("pt_aov_buffers", H.PtAovBuffers)):
        assert int(got[st]) == C.sizeof(cls), st
        assert [n for n, _ in cls._fields_] == fields[st]
        for f in fields[st]:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)
    assert list(H.AOV_BUFFERS) == fields["pt_aov_buffers"]


def test_header_declares_the_pass_and_the_libraries_export_it(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("pt_aov", "pt_aov_device", "pt_aov_finish"):
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name)
    from portrayer_amd import host
    assert "ph_renderer_aov" in host.EXPORTS and hasattr(host.lib(), "ph_renderer_aov")


def test_renderer_aov_rejects_an_unknown_buffer_name_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    cam = np.zeros(10)
    with pytest.raises(ValueError, match="albedo"):
        r.aov(cam, 8, 8, want=("depth", "albedo"))
    with pytest.raises(ValueError):
        r.aov(cam, 8, 8, want=())
    with pytest.raises(ValueError, match="into"):
        r.aov(cam, 8, 8, want=("node",), into={"node": np.zeros((8, 8), dtype=np.float64)})
