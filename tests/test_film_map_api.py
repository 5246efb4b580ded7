"""The adaptive film without a GPU (pt_film_add_map, pt_film_error, pt_film_budget_device: DESIGN 4.13): argument checks that come before any HIP call, the
ctypes structs against the header's, the declarations in the headers, the libraries and the integration guide, and Film's own argument checks. (The same errors
with a live context: tests/test_gpu_film_map.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"pt_film_map_params": ("PtFilmMapParams", ["slice", "max_samples", "seed", "sample_mode", "background_rows"], ["PtRect", "u32", "u64", "i32", "i32"]),
           "pt_film_refine_params": ("PtFilmRefineParams", ["slice", "threshold", "min_count", "max_count", "step"], ["PtRect", "f64", "u32", "u32", "u32"])}
FUNCTIONS = ("pt_film_create_moments", "pt_film_add_map", "pt_film_add_map_device", "pt_film_error", "pt_film_error_device", "pt_film_budget_device",
             "pt_test_film_moments_host", "pt_test_film_plan_host", "pt_test_film_plan")
HOST_FUNCTIONS = ("ph_renderer_film_create_moments", "ph_renderer_film_add_map", "ph_renderer_film_error", "ph_renderer_film_refine")


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
    budget = np.full((h, w), 3, dtype=np.uint32)
    err, out_budget, summary = np.full((h, w), 7.0), np.full((h, w), 7, dtype=np.uint32), np.full(2, 7, dtype=np.uint64)
    dp = lambda a: a.ctypes.data_as(H._dp)
    up = lambda a: a.ctypes.data_as(H._up)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    out = C.c_void_p(0x1234)
    for width, height in ((w, h), (0, h), (w, 0), (1 << 16, 1 << 15)):
        assert lib.pt_film_create_moments(None, width, height, C.byref(out)) == H.ERR_ARGUMENT
        assert not out.value, "a refused create leaves no handle behind"
        out = C.c_void_p(0x1234)
    assert lib.pt_film_create_moments(None, w, h, None) == H.ERR_ARGUMENT
    rect = H.PtRect(0, 0, w - 1, h - 1)
    good = H.PtFilmMapParams(rect, 8, 0, H.SAMPLE_RNG, 0)
    bad = [H.PtFilmMapParams(rect, 0, 0, H.SAMPLE_RNG, 0), H.PtFilmMapParams(rect, H.FILM_MAP_MAX + 1, 0, H.SAMPLE_RNG, 0),  # max_samples
           H.PtFilmMapParams(rect, 8, 0, 2, 0), H.PtFilmMapParams(rect, 8, 0, -1, 0),                                        # sample_mode
           H.PtFilmMapParams(rect, 8, 0, H.SAMPLE_CENTRE, 2), H.PtFilmMapParams(rect, 8, 0, H.SAMPLE_CENTRE, -1),            # background_rows
           H.PtFilmMapParams(H.PtRect(0, 0, w, h), 8, 0, H.SAMPLE_RNG, 0),                                                    # a slice corner outside
           H.PtFilmMapParams(H.PtRect(3, 3, 2, 3), 8, 0, H.SAMPLE_RNG, 0)]                                                    # an inverted slice
    refine = H.PtFilmRefineParams(rect, 0.01, 8, 32, 8)
    bad_refine = [H.PtFilmRefineParams(rect, 0.01, 8, 32, 0), H.PtFilmRefineParams(rect, 0.01, 8, 32, H.FILM_MAP_MAX + 1), H.PtFilmRefineParams(rect, 0.01, 33, 32, 8),
                  H.PtFilmRefineParams(rect, float("nan"), 8, 32, 8), H.PtFilmRefineParams(H.PtRect(0, 0, w, h), 0.01, 8, 32, 8)]
    film = C.c_void_p(0x1000)  # never dereferenced: without a context there is nothing to look it up in
    for f in (None, film):
        for p in [good] + bad:
            assert lib.pt_film_add_map(None, f, C.byref(cam), dp(bg), C.byref(p), up(budget), None) == H.ERR_ARGUMENT
            assert lib.pt_film_add_map_device(None, f, C.byref(cam), vp(bg), C.byref(p), vp(budget), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_map(None, f, None, dp(bg), C.byref(good), up(budget), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_map(None, f, C.byref(cam), None, C.byref(good), up(budget), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_map(None, f, C.byref(cam), dp(bg), None, up(budget), None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_map(None, f, C.byref(cam), dp(bg), C.byref(good), None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_add_map_device(None, f, C.byref(cam), None, None, None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_error(None, f, dp(err)) == H.ERR_ARGUMENT and lib.pt_film_error(None, f, None) == H.ERR_ARGUMENT
        assert lib.pt_film_error_device(None, f, vp(err), None) == H.ERR_ARGUMENT and lib.pt_film_error_device(None, f, None, None) == H.ERR_ARGUMENT
        for p in [refine] + bad_refine:
            assert lib.pt_film_budget_device(None, f, C.byref(p), vp(out_budget), vp(summary), None) == H.ERR_ARGUMENT
        assert lib.pt_film_budget_device(None, f, None, vp(out_budget), vp(summary), None) == H.ERR_ARGUMENT
        assert lib.pt_film_budget_device(None, f, C.byref(refine), None, vp(summary), None) == H.ERR_ARGUMENT
        assert lib.pt_film_budget_device(None, f, C.byref(refine), vp(out_budget), None, None) == H.ERR_ARGUMENT
    n = C.c_uint32(7)
    lst = np.full(64, 7, dtype=np.uint32)
    assert lib.pt_test_film_plan(None, w, h, C.byref(rect), up(budget), 8, 0, up(lst), 64, C.byref(n)) == H.ERR_ARGUMENT and n.value == 7
    assert np.all(err == 7.0) and np.all(out_budget == 7) and np.all(summary == 7) and np.all(budget == 3) and np.all(lst == 7)
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = []
    for st, (_, fields, _) in STRUCTS.items():
        lines += ['printf("%s %%zu\\n", sizeof(%s));' % (st, st)]
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in fields]
        lines += ['{ %s v; printf("%s.size.%s %%zu\\n", sizeof v.%s); }' % (st, st, f, f) for f in fields]
    lines += ['printf("PT_FILM_MAP_MAX %u\\n", (unsigned)PT_FILM_MAP_MAX);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["PT_FILM_MAP_MAX"]) == H.FILM_MAP_MAX == 4096
    for st, (cls_name, fields, _) in STRUCTS.items():
        cls = getattr(H, cls_name)
        assert int(got[st]) == C.sizeof(cls), st
        assert [n for n, _ in cls._fields_] == fields
        for f in fields:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset, (st, f)
            assert int(got["%s.size.%s" % (st, f)]) == getattr(cls, f).size, (st, f)


def test_headers_declare_the_calls_and_the_libraries_export_them(H):
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


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_them(path):
    ffi = open(os.path.join(ROOT, path)).read()
    for name in FUNCTIONS[:6]:
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi), name
    for _, (cls_name, fields, types) in STRUCTS.items():
        m = re.search(r"pub struct %s\s*\{(.*?)\}" % cls_name, ffi, flags=re.S)
        assert m, cls_name
        body = re.sub(r"//[^\n]*", "", m.group(1))
        assert re.findall(r"pub (\w+):\s*(\w+)", body) == list(zip(fields, types)), cls_name


def test_film_rejects_bad_requests_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    for w, h in ((0, 8), (8, 0), (8.0, 8), (True, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.film(w, h, moments=True)
    film = object.__new__(host.Film)  # a film that was never created: its checks must not need one
    film._h, film._r, film.width, film.height, film.moments = C.c_void_p(), r, 16, 8, True
    cam, bg, budget = np.zeros(10), np.zeros((8, 3)), np.ones((8, 16), dtype=np.uint32)
    for bad_bg in (np.zeros((8, 16)), np.zeros((16, 3)), np.zeros((8, 16, 4)), np.zeros(3)):
        with pytest.raises(ValueError, match="background"):
            film.add_map(cam, bad_bg, budget)
        with pytest.raises(ValueError, match="background"):
            film.refine(cam, bad_bg, 0.01)
    for bad in (np.ones((8, 16)), np.ones((8, 16), dtype=np.int32), np.ones((16, 8), dtype=np.uint32), np.ones(128, dtype=np.uint32), [[1] * 16] * 8, None):
        with pytest.raises(ValueError, match="budget"):
            film.add_map(cam, bg, bad)
    for bad in (0, -1, 1.5, True, "3", 4097):
        with pytest.raises(ValueError, match="max_samples"):
            film.add_map(cam, bg, budget, max_samples=bad)
    for bad in (-1, 1.5, True, "3", 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            film.add_map(cam, bg, budget, seed=bad)
        with pytest.raises(ValueError, match="seed"):
            film.refine(cam, bg, 0.01, seed=bad)
    for bad in (np.zeros((8, 16), dtype=np.float32), np.zeros((16, 8)), np.zeros((8, 16, 1)), np.zeros((8, 32))[:, ::2]):
        with pytest.raises(ValueError, match="into"):
            film.error(into=bad)
    for bad in ("1", None, float("nan"), True):
        with pytest.raises(ValueError, match="threshold"):
            film.refine(cam, bg, bad)
    for kw in ({"step": 0}, {"step": 4097}, {"step": 1.5}, {"min_count": 65}, {"min_count": -1}, {"max_count": (1 << 31) + 1}, {"max_passes": -1}, {"max_passes": True}):
        with pytest.raises(ValueError, match="|".join(kw)):
            film.refine(cam, bg, 0.01, **kw)
    film.moments = False  # a plain film has no noise estimate
    with pytest.raises(ValueError, match="moments"):
        film.error()
    with pytest.raises(ValueError, match="moments"):
        film.refine(cam, bg, 0.01)
    film.close()  # nothing to destroy
