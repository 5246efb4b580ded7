"""The radiance pass without a GPU: argument checks that come before any HIP call, the ctypes struct against the header's, the declarations in the
header, the libraries and the shim, and Renderer.radiance's own argument checks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["n", "reorder", "background_per_ray", "seed", "stream_base", "sample"]
FUNCTIONS = ("pt_radiance", "pt_radiance_device", "pt_radiance_finish")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_every_argument_error_comes_before_any_hip_call(H):
    """No GPU and no context here: a NULL context, alone and together with every other argument error of the header, is PT_ERR_ARGUMENT - no call
    dereferences the context or reaches the runtime. (The same errors with a live context: tests/test_gpu_radiance.py::test_argument_errors.)"""
    lib = H.lib()
    n = 4
    o, d, bg, rgb = np.zeros((n, 3)), np.ones((n, 3)), np.zeros(3), np.zeros((n, 3))
    dp = lambda a: a.ctypes.data_as(H._dp)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    good = H.PtRadianceParams(n, 0, 0, 0, 0, 0)
    cases = [
        (good, o, d, bg, rgb),                                                            # only the context is NULL
        (None, o, d, bg, rgb),                                                            # params
        (good, None, d, bg, rgb), (good, o, None, bg, rgb), (good, o, d, None, rgb),      # an input
        (good, o, d, bg, None),                                                           # the output
        (H.PtRadianceParams(H.RAYS_MAX + 1, 0, 0, 0, 0, 0), o, d, bg, rgb),               # n beyond the limit
        (H.PtRadianceParams(n, 2, 0, 0, 0, 0), o, d, bg, rgb), (H.PtRadianceParams(n, -1, 0, 0, 0, 0), o, d, bg, rgb),  # reorder
        (H.PtRadianceParams(n, 0, 2, 0, 0, 0), o, d, bg, rgb), (H.PtRadianceParams(n, 0, -1, 0, 0, 0), o, d, bg, rgb),  # background_per_ray
        (H.PtRadianceParams(0, 0, 0, 0, 0, 0), o, d, bg, rgb),                            # n = 0 is fine only with a context
    ]
    for p, po, pd, pb, pr in cases:
        pp = C.byref(p) if p is not None else None
        host = [dp(a) if a is not None else None for a in (po, pd, pb, pr)]
        dev = [vp(a) if a is not None else None for a in (po, pd, pb, pr)]
        assert lib.pt_radiance(None, pp, *host, None) == H.ERR_ARGUMENT
        assert lib.pt_radiance_device(None, pp, *dev, None) == H.ERR_ARGUMENT
    assert lib.pt_radiance_finish(None, None) == H.ERR_ARGUMENT
    assert not rgb.any()
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_struct_has_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    st = "pt_radiance_params"
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (st, st)]
    lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in FIELDS]
    lines += ['{ %s v; printf("size.%s %%zu\\n", sizeof v.%s); }' % (st, f, f) for f in FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    cls = H.PtRadianceParams
    assert int(got[st]) == C.sizeof(cls)
    assert [n for n, _ in cls._fields_] == FIELDS
    for f in FIELDS:
        assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, f
        assert int(got["size.%s" % f]) == getattr(cls, f).size, f


def test_header_declares_the_pass_and_the_libraries_export_it(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name)
    assert not H.missing_symbols()
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        assert re.search(r"\bint ph_renderer_radiance\s*\(", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))
    from portrayer_amd import host
    assert "ph_renderer_radiance" in host.EXPORTS and hasattr(host.lib(), "ph_renderer_radiance")


def test_the_shim_and_the_integration_guide_declare_the_pass():
    for path in (os.path.join(ROOT, "shim", "src", "hip_ffi.rs"), os.path.join(ROOT, "INTEGRATION.md")):
        ffi = open(path).read()
        for name in FUNCTIONS:
            assert re.search(r"\bpub fn %s\s*\(" % name, ffi), (path, name)
        m = re.search(r"pub struct PtRadianceParams\s*\{(.*?)\}", ffi, flags=re.S)
        assert m, path
        body = re.sub(r"//[^\n]*", "", m.group(1))
        assert re.findall(r"pub (\w+):\s*(\w+)", body) == list(zip(FIELDS, ["u64", "i32", "i32", "u64", "u64", "u32"])), path


def test_renderer_radiance_rejects_bad_requests_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.radiance(o, np.ones((7, 3)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.radiance(np.zeros((8, 2)), np.ones((8, 2)))
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.radiance(np.zeros(24), np.ones(24))
    with pytest.raises(ValueError, match="float64"):
        r.radiance(o.astype(np.float32), d)
    with pytest.raises(ValueError, match="background"):
        r.radiance(o, d, background=(0.0, 0.0))
    with pytest.raises(ValueError, match="background"):
        r.radiance(o, d, background=np.zeros((7, 3)))
    with pytest.raises(ValueError, match="background"):
        r.radiance(o, d, background=np.zeros((8, 3, 1)))
    for name in ("seed", "sample", "stream_base"):
        for bad in (-1, 1.5, True, "3"):
            with pytest.raises(ValueError, match=name):
                r.radiance(o, d, **{name: bad})
    with pytest.raises(ValueError, match="sample"):
        r.radiance(o, d, sample=1 << 32)
    with pytest.raises(ValueError, match="seed"):
        r.radiance(o, d, seed=1 << 64)
    for bad in (2, -1, 1.0, "1", None):
        with pytest.raises(ValueError, match="reorder"):
            r.radiance(o, d, reorder=bad)
    with pytest.raises(ValueError, match="into"):
        r.radiance(o, d, into=np.zeros((8, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="into"):
        r.radiance(o, d, into=np.zeros((7, 3)))
    with pytest.raises(ValueError, match="into"):
        r.radiance(o, d, into=np.zeros((3, 8)).T)
