"""The ray-query pass without a GPU: argument checks that come before any HIP call, the ctypes structs against the header's, the
declarations in the header, the libraries and the shim, and Renderer.rays' own argument checks."""
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


def _call_args(H, n=4):
    o, d = np.zeros((n, 3)), np.ones((n, 3))
    t, occ = np.zeros(n), np.zeros(n, dtype=np.uint8)
    return o, d, t, occ


def test_every_argument_error_comes_before_any_hip_call(H):
    """No GPU and no context here: a NULL context, alone and together with every other argument error of the header, is PT_ERR_ARGUMENT - no call
    dereferences the context or reaches the runtime. (The same errors with a live context: tests/test_gpu_rays.py::test_argument_errors.)"""
    lib = H.lib()
    o, d, t, occ = _call_args(H)
    dp = lambda a: a.ctypes.data_as(H._dp)
    good_p = H.PtRaysParams(4, 0, 0)
    good_b = H.PtRaysBuffers(t=dp(t))
    occ_b = H.PtRaysBuffers(occluded=occ.ctypes.data_as(H._u8p))
    cases = [
        (good_p, dp(o), dp(d), good_b),                                   # only the context is NULL
        (None, dp(o), dp(d), good_b),                                     # params
        (good_p, None, dp(d), good_b), (good_p, dp(o), None, good_b),     # an input
        (good_p, dp(o), dp(d), H.PtRaysBuffers()), (good_p, dp(o), dp(d), None),  # no buffer requested
        (H.PtRaysParams(H.RAYS_MAX + 1, 0, 0), dp(o), dp(d), good_b),     # n beyond the limit
        (H.PtRaysParams(4, 2, 0), dp(o), dp(d), occ_b), (H.PtRaysParams(4, -1, 0), dp(o), dp(d), occ_b),  # any_hit
        (H.PtRaysParams(4, 0, 2), dp(o), dp(d), good_b), (H.PtRaysParams(4, 0, -1), dp(o), dp(d), good_b),  # reorder
        (H.PtRaysParams(4, 1, 0), dp(o), dp(d), good_b),                  # an occlusion query asking for more than `occluded`
        (H.PtRaysParams(0, 0, 0), dp(o), dp(d), good_b),                  # n = 0 is fine only with a context
    ]
    for p, po, pd, b in cases:
        pp = C.byref(p) if p is not None else None
        pb = C.byref(b) if b is not None else None
        assert lib.pt_rays(None, pp, po, pd, pb, None) == H.ERR_ARGUMENT
        assert lib.pt_rays_device(None, pp, po, pd, pb, None) == H.ERR_ARGUMENT
    assert lib.pt_rays_finish(None, None) == H.ERR_ARGUMENT
    assert not t.any() and not occ.any()
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    fields = {"pt_rays_params": ["n", "any_hit", "reorder"], "pt_rays_buffers": ["t", "position", "normal", "node", "sub", "material", "occluded"]}
    lines = ['printf("PT_RAYS_MAX %llu\\n", (unsigned long long)PT_RAYS_MAX);']
    for st, fs in fields.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (st, st))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for st, cls in (("pt_rays_params", H.PtRaysParams), ("pt_rays_buffers", H.PtRaysBuffers)):
        assert int(got[st]) == C.sizeof(cls), st
        assert [n for n, _ in cls._fields_] == fields[st]
        for f in fields[st]:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)
    assert list(H.RAYS_BUFFERS) == fields["pt_rays_buffers"]
    assert int(got["PT_RAYS_MAX"]) == H.RAYS_MAX


def test_header_declares_the_pass_and_the_libraries_export_it(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("pt_rays", "pt_rays_device", "pt_rays_finish"):
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name)
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        assert re.search(r"\bint ph_renderer_rays\s*\(", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))
    from portrayer_amd import host
    assert "ph_renderer_rays" in host.EXPORTS and hasattr(host.lib(), "ph_renderer_rays")


def test_the_shim_declares_the_pass():
    ffi = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    for name in ("pt_rays", "pt_rays_device", "pt_rays_finish"):
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi), name
    for st, fs in (("PtRaysParams", ["n", "any_hit", "reorder"]), ("PtRaysBuffers", ["t", "position", "normal", "node", "sub", "material", "occluded"])):
        m = re.search(r"pub struct %s\s*\{(.*?)\}" % st, ffi, flags=re.S)
        assert m, st
        assert re.findall(r"pub (\w+):", re.sub(r"//[^\n]*", "", m.group(1))) == fs, st


def test_renderer_rays_rejects_bad_requests_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="albedo"):
        r.rays(o, d, want=("t", "albedo"))
    with pytest.raises(ValueError):
        r.rays(o, d, want=())
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.rays(o, np.ones((7, 3)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.rays(np.zeros((8, 2)), np.ones((8, 2)))
    with pytest.raises(ValueError, match="float64"):
        r.rays(o.astype(np.float32), d)
    with pytest.raises(ValueError, match="any_hit"):
        r.rays(o, d, any_hit=True, want=("occluded", "t"))
    with pytest.raises(ValueError, match="any_hit"):
        r.rays(o, d, any_hit=True, want=("node",))
    with pytest.raises(ValueError, match="into"):
        r.rays(o, d, want=("node",), into={"node": np.zeros(8, dtype=np.float64)})
    with pytest.raises(ValueError, match="into"):
        r.rays(o, d, want=("position",), into={"position": np.zeros((8,))})
