"""The film without a GPU: argument checks that come before any HIP call, the ctypes struct against the header's, the declarations in the headers, the
libraries and the integration guide, and Film's own argument checks. (The same errors with a live context: tests/test_gpu_film.py::test_argument_errors.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["slice", "samples", "seed", "sample_mode", "background_rows"]
FUNCTIONS = ("pt_film_create", "pt_film_destroy", "pt_film_reset", "pt_film_add", "pt_film_add_device", "pt_film_resolve", "pt_film_resolve_device", "pt_film_counts",
             "pt_test_film_fold_host")
HOST_FUNCTIONS = ("ph_renderer_film_create", "ph_renderer_film_destroy", "ph_renderer_film_reset", "ph_renderer_film_add", "ph_renderer_film_resolve", "ph_renderer_film_counts")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_every_argument_error_comes_before_any_hip_call(H):
    """No GPU and no context here: a NULL context or a NULL film, alone and together with every other argument error of the header, is PT_ERR_ARGUMENT - no
    call dereferences either or reaches the runtime, and nothing is written."""
    lib = H.lib()
    w, h = 16, 8
    cam, bg = H.PtCamera(), np.zeros((h, w, 3))
    rgb, linear, counts = np.full((h, w, 3), 7, dtype=np.uint8), np.full((h, w, 3), 7.0), np.full((h, w), 7, dtype=np.uint32)
    dp = lambda a: a.ctypes.data_as(H._dp)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    out = C.c_void_p(0x1234)
    for width, height in ((w, h), (0, h), (w, 0), (1 << 16, 1 << 15)):
        assert lib.pt_film_create(None, width, height, C.byref(out)) == H.ERR_ARGUMENT
        assert not out.value, "a refused create leaves no handle behind"
        out = C.c_void_p(0x1234)
    assert lib.pt_film_create(None, w, h, None) == H.ERR_ARGUMENT
    rect = H.PtRect(0, 0, w - 1, h - 1)
    good = H.PtFilmParams(rect, 1, 0, H.SAMPLE_RNG, 0)
    bad = [H.PtFilmParams(rect, 0, 0, H.SAMPLE_RNG, 0),                                               # samples == 0
           H.PtFilmParams(rect, 1, 0, 2, 0), H.PtFilmParams(rect, 1, 0, -1, 0),                       # sample_mode
           H.PtFilmParams(rect, 1, 0, H.SAMPLE_CENTRE, 2), H.PtFilmParams(rect, 1, 0, H.SAMPLE_CENTRE, -1),  # background_rows
           H.PtFilmParams(H.PtRect(0, 0, w, h), 1, 0, H.SAMPLE_RNG, 0),                               # a slice corner outside
           H.PtFilmParams(H.PtRect(3, 3, 2, 3), 1, 0, H.SAMPLE_RNG, 0),                               # an inverted slice is fine only with a context and a film
           H.PtFilmParams(rect, 0xFFFFFFFF, 0, H.SAMPLE_RNG, 0)]                                      # past 2^31 whatever the film holds
    film = C.c_void_p(0x1000)  # never dereferenced: without a context there is nothing to look it up in
    for f in (None, film):
        for p in [good] + bad:
            assert lib.pt_film_add(None, f, C.byref(cam), dp(bg), C.byref(p), None) == H.ERR_ARGUMENT
            assert lib.pt_film_add_device(None, f, C.byref(cam), vp(bg), C.byref(p), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add(None, f, None, dp(bg), C.byref(good), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add(None, f, C.byref(cam), None, C.byref(good), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add(None, f, C.byref(cam), dp(bg), None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_device(None, f, C.byref(cam), None, None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_destroy(None, f) == H.ERR_ARGUMENT and lib.pt_film_reset(None, f) == H.ERR_ARGUMENT
        assert lib.pt_film_resolve(None, f, rgb.ctypes.data_as(H._u8p), dp(linear)) == H.ERR_ARGUMENT
        assert lib.pt_film_resolve(None, f, None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_resolve_device(None, f, vp(rgb), vp(linear), None) == H.ERR_ARGUMENT
        assert lib.pt_film_resolve_device(None, f, None, None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_counts(None, f, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.ERR_ARGUMENT
        assert lib.pt_film_counts(None, f, None) == H.ERR_ARGUMENT
    assert np.all(rgb == 7) and np.all(linear == 7.0) and np.all(counts == 7)
    assert lib.pt_radiance_finish(None, None) == H.ERR_ARGUMENT  # what closes a film pass
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_struct_has_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    st = "pt_film_params"
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (st, st)]
    lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in FIELDS]
    lines += ['{ %s v; printf("size.%s %%zu\\n", sizeof v.%s); }' % (st, f, f) for f in FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    cls = H.PtFilmParams
    assert int(got[st]) == C.sizeof(cls)
    assert [n for n, _ in cls._fields_] == FIELDS
    for f in FIELDS:
        assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, f
        assert int(got["size.%s" % f]) == getattr(cls, f).size, f


def test_headers_declare_the_film_and_the_libraries_export_it(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name), name
    assert not H.missing_symbols()
    assert re.search(r"^#define\s+PT_ABI_VERSION\s+8\b", text, flags=re.M)
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        host_text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    from portrayer_amd import host
    for name in HOST_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % name, host_text) and name in host.EXPORTS and hasattr(host.lib(), name), name


def test_the_integration_guide_declares_the_film():
    ffi = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in FUNCTIONS[:-1]:
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi), name
    m = re.search(r"pub struct PtFilmParams\s*\{(.*?)\}", ffi, flags=re.S)
    assert m
    body = re.sub(r"//[^\n]*", "", m.group(1))
    assert re.findall(r"pub (\w+):\s*(\w+)", body) == list(zip(FIELDS, ["PtRect", "u32", "u64", "i32", "i32"]))


def test_film_rejects_bad_requests_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    for w, h in ((0, 8), (8, 0), (-1, 8), (8.0, 8), (True, 8), ("8", 8), (1 << 32, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.film(w, h)
    film = object.__new__(host.Film)  # a film that was never created: its checks must not need one
    film._h, film._r, film.width, film.height = C.c_void_p(), r, 16, 8
    cam = np.zeros(10)
    for bg in (np.zeros((8, 16)), np.zeros((16, 3)), np.zeros((8, 16, 4)), np.zeros(3)):
        with pytest.raises(ValueError, match="background"):
            film.add(cam, bg)
    for bad in (0, -1, 1.5, True, "3", (1 << 31) + 1):
        with pytest.raises(ValueError, match="samples"):
            film.add(cam, np.zeros((8, 3)), samples=bad)
    for bad in (-1, 1.5, True, "3", 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            film.add(cam, np.zeros((8, 3)), seed=bad)
    with pytest.raises(ValueError, match="into"):
        film.resolve(into=np.zeros((8, 16, 3)))
    with pytest.raises(ValueError, match="into"):
        film.resolve(into=np.zeros((16, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="linear_into"):
        film.resolve(linear_into=np.zeros((8, 16, 3), dtype=np.float32))
    film.close()  # nothing to destroy
