"""The gather pass without a GPU: the header's declarations and both libraries' exports, the ctypes structs against the header's, every refusal that comes
before a HIP call, Renderer.gather's and Renderer.gather_camera's own argument checks, and the declarations in INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_gather", "pt_gather_device", "pt_gather_finish")
HOST_CALLS = ("ph_renderer_gather", "ph_renderer_gather_camera")
PARAM_FIELDS = ["n", "samples", "pass", "seed", "first_index", "bias", "flags", "eye"]  # the header's names; ctypes says pass_index (`pass` is a keyword)
BUFFER_FIELDS = ["sum", "valid"]


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
    assert C.sizeof(H.PtAoParams) == 80 and C.sizeof(H.PtRadianceParams) == 40 and list(H.AO_BUFFERS) == ["occluded", "valid", "bent"]
    assert H.AO_MAX == 1 << 24


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("params %zu\\n", sizeof(pt_gather_params));', 'printf("buffers %zu\\n", sizeof(pt_gather_buffers));']
    lines += ['printf("p.%s %%zu\\n", offsetof(pt_gather_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['printf("b.%s %%zu\\n", offsetof(pt_gather_buffers, %s));' % (f, f) for f in BUFFER_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(H.PtGatherParams) == 72 and int(got["buffers"]) == C.sizeof(H.PtGatherBuffers) == 16
    assert [n for n, _ in H.PtGatherParams._fields_] == [f if f != "pass" else "pass_index" for f in PARAM_FIELDS]
    assert [n for n, _ in H.PtGatherBuffers._fields_] == BUFFER_FIELDS == list(H.GATHER_BUFFERS)
    for f in PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(H.PtGatherParams, f if f != "pass" else "pass_index").offset, f
    for f in BUFFER_FIELDS:
        assert int(got["b." + f]) == getattr(H.PtGatherBuffers, f).offset, f


def test_every_refusal_before_a_hip_call_is_an_argument_error_and_writes_nothing(H):
    """pt_gather's checks run in the header's order and a NULL context is the first of them, so with no GPU every call below is PT_ERR_ARGUMENT; the refusals of
    the parameter block are repeated on a live context, where their own words can be read, by tests/test_gpu_gather.py. Nothing is written either way."""
    lib = H.lib()
    P, N, bg = np.zeros((4, 3)), np.ones((4, 3)), np.array([0.25, 0.5, 1.0])
    total, valid = np.full((4, 3), 7.0), np.full(4, 7, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ok = dict(n=4, samples=16, pass_index=0, seed=0, first_index=0, bias=0.0, flags=0)
    b = H.PtGatherBuffers(sum=dp(total), valid=valid.ctypes.data_as(H._u8p))
    p = H.PtGatherParams(**ok)
    assert lib.pt_gather(None, C.byref(p), dp(P), dp(N), dp(bg), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_gather_device(None, C.byref(p), P.ctypes.data, N.ctypes.data, dp(bg), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_gather_finish(None, None) == H.ERR_ARGUMENT
    bad = [dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=128), dict(bias=-1.0), dict(bias=float("inf")), dict(bias=float("nan")), dict(flags=2),
           dict(flags=H.AO_FACE_EYE | 4)]
    for change in bad:
        q = H.PtGatherParams(**dict(ok, **change))
        assert lib.pt_gather(None, C.byref(q), dp(P), dp(N), dp(bg), C.byref(b), None) == H.ERR_ARGUMENT, change
        assert lib.pt_gather_device(None, C.byref(q), P.ctypes.data, N.ctypes.data, dp(bg), C.byref(b), None) == H.ERR_ARGUMENT, change
    for args in ((None, dp(P), dp(N), dp(bg), C.byref(b)), (C.byref(p), None, dp(N), dp(bg), C.byref(b)), (C.byref(p), dp(P), None, dp(bg), C.byref(b)),
                 (C.byref(p), dp(P), dp(N), None, C.byref(b)), (C.byref(p), dp(P), dp(N), dp(bg), None), (C.byref(p), dp(P), dp(N), dp(bg), C.byref(H.PtGatherBuffers()))):
        assert lib.pt_gather(None, *args, None) == H.ERR_ARGUMENT
    assert np.all(total == 7.0) and np.all(valid == 7)


def test_the_refusals_stand_in_the_source_in_the_headers_order_before_the_first_hip_call():
    """What a machine without a GPU can say about the refusals of a LIVE context: pt_gather_check holds every one of them, in the order the header lists them,
    calls nothing of HIP, and both entry points ask it before anything else."""
    api = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_api.hip")).read()
    start = api.index("static int pt_gather_check(")
    check = api[start:api.index("\n}\n", start)]
    assert "hip" not in check.replace("hip_stream", "") and "PT_HIP" not in check
    order = ["NULL context, params, positions, normals, background or buffers", "no output buffer asked for", "more than PT_AO_MAX points", "samples must be a power of two",
             "bias must be finite and not negative", "unknown flags", "PT_AO_FACE_EYE needs a finite eye", "PT_ERR_NO_SCENE", "c->radiance.pass.pending"]
    at = [check.index(w) for w in order]
    assert at == sorted(at)
    for entry in ('extern "C" int pt_gather(', 'extern "C" int pt_gather_device('):
        s = api.index(entry)
        body = api[s:api.index("\n}\n", s)]
        assert body.index("pt_gather_check(") < body.index("PT_HIP(") and body.index("p->n == 0) return PT_OK") < body.index("PT_HIP(")
    assert 'extern "C" int pt_gather_finish(pt_context* c, double* kernel_ms) { return pt_radiance_finish(c, kernel_ms); }' in api


def _NoLibrary():
    """A Renderer with no scene and no context: any library call would fail on the null handle."""
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):
            self._h = C.c_void_p()
            self.scene = None
    return NoLibrary()


def test_renderer_gather_rejects_bad_arguments_before_any_library_call():
    r = _NoLibrary()
    P, N = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="want"):
        r.gather(P, N, want=("sum", "mean"))
    with pytest.raises(ValueError, match="want"):
        r.gather(P, N, want=())
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.gather(P, N[:7])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.gather(P.ravel(), N.ravel())
    with pytest.raises(ValueError, match="float64"):
        r.gather(P.astype(np.float32), N.astype(np.float32))
    for S in (0, 3, 128, 16.0, True, None):
        with pytest.raises(ValueError, match="samples"):
            r.gather(P, N, samples=S)
    for bias in (-1e-9, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="bias"):
            r.gather(P, N, bias=bias)
    for name in ("seed", "pass_index", "first_index"):
        for v in (-1, 1.5, True, 1 << 64):
            with pytest.raises(ValueError, match=name):
                r.gather(P, N, **{name: v})
    with pytest.raises(ValueError, match="pass_index"):
        r.gather(P, N, pass_index=1 << 32)
    for eye in ((0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
        with pytest.raises(ValueError, match="eye"):
            r.gather(P, N, eye=eye)
    for bg in ((0.0, 0.0), np.zeros((8, 3)), 1.0):
        with pytest.raises(ValueError, match="background"):
            r.gather(P, N, background=bg)
    with pytest.raises(ValueError, match="into"):
        r.gather(P, N, want=("sum",), into={"sum": np.zeros((8, 3), dtype=np.float32)})
    with pytest.raises(ValueError, match="into"):
        r.gather(P, N, want=("sum",), into={"sum": np.zeros(8)})
    with pytest.raises(ValueError, match="into"):
        r.gather(P, N, want=("valid",), into={"valid": [0] * 8})
    with pytest.raises(TypeError):
        r.gather(P, N, radius=1.0)  # a gather ray is unbounded: there is no such argument


def test_renderer_gather_camera_rejects_bad_arguments_before_any_library_call():
    r = _NoLibrary()
    cam = np.zeros(10)
    for w, h in ((0, 8), (8, 0), (8.0, 8), (True, 8), (-1, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.gather_camera(cam, w, h)
    with pytest.raises(ValueError, match="points"):
        r.gather_camera(cam, 8192, 4096)  # 2^25 pixels > PT_AO_MAX
    with pytest.raises(ValueError, match="samples"):
        r.gather_camera(cam, 8, 8, samples=5)
    with pytest.raises(ValueError, match="bias"):
        r.gather_camera(cam, 8, 8, bias=-1.0)
    with pytest.raises(ValueError, match="background"):
        r.gather_camera(cam, 8, 8, background=(1.0,))
    with pytest.raises(ValueError, match="into"):
        r.gather_camera(cam, 8, 4, want=("sum",), into={"sum": np.zeros((8, 4, 3))})
    with pytest.raises(ValueError, match="cam10"):
        r.gather_camera(np.zeros(9), 8, 8)
    with pytest.raises(ValueError, match="want"):
        r.gather_camera(cam, 8, 8, want=("mean",))


def test_the_docstrings_say_what_the_mean_estimates():
    from portrayer_amd import host
    for fn in (host.Renderer.gather, host.Renderer.gather_camera):
        assert re.search(r"irradiance estimate .*pi x mean", fn.__doc__), fn.__name__


def test_the_host_library_refuses_null_and_oversized_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    p = H.PtGatherParams(4, 16, 0, 0, 0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    total = np.zeros((4, 3))
    b = H.PtGatherBuffers(sum=total.ctypes.data_as(H._dp))
    P, bg, cam = np.zeros((4, 3)), np.zeros(3), np.zeros(10)
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.ph_renderer_gather(None, C.byref(p), dp(P), dp(P), dp(bg), C.byref(b), None) == -1
    assert lib.ph_renderer_gather_camera(None, dp(cam), 2, 2, C.byref(p), dp(bg), C.byref(b), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtGatherParams\s*\{[^}]*pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,\s*pub bias: f64, "
                     r"pub flags: u32, pub eye: \[f64; 3\],\s*\}", text)
    assert re.search(r"pub struct PtGatherBuffers\s*\{[^}]*pub sum: \*mut f64, pub valid: \*mut u8,\s*\}", text)
    for name in HIP_CALLS:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_gather\([^)]*params: \*const PtGatherParams, positions: \*const f64, normals: \*const f64, background: \*const f64,\s*"
                     r"host_out: \*const PtGatherBuffers,", text)
