"""The denoiser without a GPU (pt_film_denoise, pt_film_denoise_device, pt_test_denoise_host: DESIGN 4.14): argument checks that come before any HIP call, the
ctypes structs against the header's, the declarations in the headers, the libraries and the integration guide, and Film.denoise's own argument checks. (The same
errors with a live context, and the filter itself: tests/test_gpu_denoise.py; the contract's arithmetic: tests/test_denoise_host.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"pt_denoise_params": ("PtDenoiseParams", ["iterations", "flags", "sigma_color", "sigma_plane", "normal_power_log2"], ["i32", "u32", "f64", "f64", "i32"]),
           "pt_denoise_guides": ("PtDenoiseGuides", ["position", "normal", "node"], ["*const f64", "*const f64", "*const i32"])}
FUNCTIONS = ("pt_film_denoise", "pt_film_denoise_device", "pt_test_denoise_host")
HOST_FUNCTIONS = ("ph_renderer_film_denoise",)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_every_argument_error_comes_before_any_hip_call(H):
    """No GPU and no context here: a NULL context or a NULL film, alone and together with every other argument error of the header, is PT_ERR_ARGUMENT - no
    call dereferences either or reaches the runtime, and nothing is written."""
    lib = H.lib()
    w, h = 16, 8
    node, normal, position = np.zeros((h, w), dtype=np.int32), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    rgb, linear, variance = np.full((h, w, 3), 7, dtype=np.uint8), np.full((h, w, 3), 7.0), np.full((h, w), 7.0)
    full = H.PtDenoiseGuides(position.ctypes.data, normal.ctypes.data, node.ctypes.data)
    good = H.PtDenoiseParams(5, 0, 2.0, 0.05, 5)
    nan, inf = float("nan"), float("inf")
    bad = [H.PtDenoiseParams(0, 0, 2.0, 0.05, 5), H.PtDenoiseParams(9, 0, 2.0, 0.05, 5), H.PtDenoiseParams(5, 2, 2.0, 0.05, 5), H.PtDenoiseParams(5, 0, -1.0, 0.05, 5),
           H.PtDenoiseParams(5, 0, nan, 0.05, 5), H.PtDenoiseParams(5, 0, inf, 0.05, 5), H.PtDenoiseParams(5, 0, 2.0, -1.0, 5), H.PtDenoiseParams(5, 0, 2.0, nan, 5),
           H.PtDenoiseParams(5, 0, 2.0, inf, 5), H.PtDenoiseParams(5, 0, 2.0, 0.05, -2), H.PtDenoiseParams(5, 0, 2.0, 0.05, 8)]
    bad_guides = [H.PtDenoiseGuides(position.ctypes.data, normal.ctypes.data, None), H.PtDenoiseGuides(position.ctypes.data, None, node.ctypes.data),
                  H.PtDenoiseGuides(None, normal.ctypes.data, node.ctypes.data)]
    dp, u8 = (lambda a: a.ctypes.data_as(H._dp)), (lambda a: a.ctypes.data_as(H._u8p))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    film = C.c_void_p(0x1000)  # never dereferenced: without a context there is nothing to look it up in
    for f in (None, film):
        for p in [good] + bad:
            for g in [full] + bad_guides:
                assert lib.pt_film_denoise(None, f, C.byref(p), C.byref(g), u8(rgb), dp(linear), dp(variance)) == H.ERR_ARGUMENT
                assert lib.pt_film_denoise_device(None, f, C.byref(p), C.byref(g), vp(rgb), vp(linear), vp(variance), None) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise(None, f, None, C.byref(full), u8(rgb), dp(linear), dp(variance)) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise(None, f, C.byref(good), None, u8(rgb), dp(linear), dp(variance)) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise(None, f, C.byref(good), C.byref(full), None, None, None) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise_device(None, f, None, C.byref(full), vp(rgb), vp(linear), vp(variance), None) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise_device(None, f, C.byref(good), None, vp(rgb), vp(linear), vp(variance), None) == H.ERR_ARGUMENT
        assert lib.pt_film_denoise_device(None, f, C.byref(good), C.byref(full), None, None, None, None) == H.ERR_ARGUMENT
    assert np.all(rgb == 7) and np.all(linear == 7.0) and np.all(variance == 7.0)
    assert lib.pt_abi_version() == 8  # additive: the ABI number stays


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = []
    for st, (_, fields, _) in STRUCTS.items():
        lines += ['printf("%s %%zu\\n", sizeof(%s));' % (st, st)]
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f) for f in fields]
        lines += ['{ %s v; printf("%s.size.%s %%zu\\n", sizeof v.%s); }' % (st, st, f, f) for f in fields]
    lines += ['printf("PT_DENOISE_SAME_NODE %u\\n", (unsigned)PT_DENOISE_SAME_NODE);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["PT_DENOISE_SAME_NODE"]) == H.DENOISE_SAME_NODE == 1
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


def test_the_contract_header_says_whose_the_work_buffers_are():
    text = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_denoise.h")).read()
    assert "32 bytes per pixel" in text and "BELONG TO THE FILM" in text and "freed with the film" in text
    assert re.search(r"#define\s+PT_DENOISE_EPS\s+1e-12\b", text)


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_them(path):
    ffi = open(os.path.join(ROOT, path)).read()
    for name in FUNCTIONS[:2]:
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi), name
    for _, (cls_name, fields, types) in STRUCTS.items():
        m = re.search(r"pub struct %s\s*\{(.*?)\}" % cls_name, ffi, flags=re.S)
        assert m, cls_name
        body = re.sub(r"//[^\n]*", "", m.group(1))
        assert re.findall(r"pub (\w+):\s*([*\w ]+?)\s*,", body) == list(zip(fields, types)), cls_name


def test_film_denoise_rejects_bad_requests_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    film = object.__new__(host.Film)  # a film that was never created: its checks must not need one
    film._h, film._r, film.width, film.height, film.moments = C.c_void_p(), NoLibrary(), 16, 8, True
    cam = np.zeros(10)
    for bad in (0, 9, -1, 1.5, True, "3", None):
        with pytest.raises(ValueError, match="iterations"):
            film.denoise(cam, iterations=bad)
    for bad in (-1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="sigma_color"):
            film.denoise(cam, sigma_color=bad)
        with pytest.raises(ValueError, match="sigma_plane"):
            film.denoise(cam, sigma_plane=bad)
    for bad in (0, 3, 256, -2, 2.0, True, "32"):
        with pytest.raises(ValueError, match="normal_power"):
            film.denoise(cam, normal_power=bad)
    node, normal, position = np.zeros((8, 16), dtype=np.int32), np.zeros((8, 16, 3)), np.zeros((8, 16, 3))
    for bad in ([node], "node", {"normal": normal}, {"node": node.astype(np.int64), "normal": normal}, {"node": node.T, "normal": normal}, {"node": node},
                {"node": node, "normal": normal.astype(np.float32)}, {"node": node, "normal": normal[:, :, :2]}):
        with pytest.raises(ValueError, match="guides"):
            film.denoise(cam, guides=bad)
    with pytest.raises(ValueError, match="guides"):
        film.denoise(cam, sigma_plane=0.05, guides={"node": node, "normal": normal})  # the plane weight reads positions
    for kw, bad in (("into", np.zeros((8, 16, 3))), ("into", np.zeros((16, 8, 3), dtype=np.uint8)), ("linear_into", np.zeros((8, 16, 3), dtype=np.float32)),
                    ("linear_into", np.zeros((8, 16))), ("variance_into", np.zeros((8, 16, 3))), ("variance_into", np.zeros((8, 32))[:, ::2])):
        with pytest.raises(ValueError, match=kw):
            film.denoise(cam, **{kw: bad})
    for bad in (None, np.zeros(9), np.zeros((2, 5))):
        with pytest.raises(ValueError, match="cam10"):
            film.denoise(bad)
    film.moments = False  # a plain film has no noise estimate: the colour weight must be off
    with pytest.raises(ValueError, match="moments"):
        film.denoise(cam)
    film.close()  # nothing to destroy
