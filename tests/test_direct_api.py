"""The direct-light pass without a GPU: the header's declarations and both libraries' exports, the ctypes structs against the header's, every refusal that comes
before a HIP call and their order in the source, Renderer.direct's, direct_camera's and direct_chart's own argument checks, and the declarations in
INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_direct", "pt_direct_device", "pt_direct_finish", "pt_test_direct_host")
HOST_CALLS = ("ph_renderer_direct", "ph_renderer_direct_camera", "ph_renderer_direct_chart")
PARAM_FIELDS = ["n", "samples", "pass", "seed", "first_index", "bias", "flags", "eye"]  # the header's names; ctypes says pass_index (`pass` is a keyword)
BUFFER_FIELDS = ["sum", "lit", "valid"]


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
    assert H.AO_FACE_EYE == 1 and H.DIRECT_TO_LIGHT == 2 and list(H.AO_BUFFERS) == ["occluded", "valid", "bent"] and list(H.GATHER_BUFFERS) == ["sum", "valid"]
    assert C.sizeof(H.PtDirectParams) == C.sizeof(H.PtGatherParams) == C.sizeof(H.PtAoParams) - 8, "pt_ao_params without the radius"


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("params %zu\\n", sizeof(pt_direct_params));', 'printf("buffers %zu\\n", sizeof(pt_direct_buffers));',
             'printf("TO_LIGHT %u\\n", (unsigned)PT_DIRECT_TO_LIGHT);', 'printf("FACE_EYE %u\\n", (unsigned)PT_AO_FACE_EYE);']
    lines += ['printf("p.%s %%zu\\n", offsetof(pt_direct_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['printf("b.%s %%zu\\n", offsetof(pt_direct_buffers, %s));' % (f, f) for f in BUFFER_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(H.PtDirectParams) and int(got["buffers"]) == C.sizeof(H.PtDirectBuffers)
    assert int(got["TO_LIGHT"]) == H.DIRECT_TO_LIGHT and int(got["FACE_EYE"]) == H.AO_FACE_EYE
    assert [n for n, _ in H.PtDirectParams._fields_] == [f if f != "pass" else "pass_index" for f in PARAM_FIELDS]
    assert [n for n, _ in H.PtDirectBuffers._fields_] == BUFFER_FIELDS == list(H.DIRECT_BUFFERS)
    for f in PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(H.PtDirectParams, f if f != "pass" else "pass_index").offset, f
    for f in BUFFER_FIELDS:
        assert int(got["b." + f]) == getattr(H.PtDirectBuffers, f).offset, f


def test_null_arguments_are_argument_errors_before_any_hip_call(H):
    lib = H.lib()
    P, N, lit = np.zeros((4, 3)), np.ones((4, 3)), np.full(4, 7, dtype=np.uint32)
    p = H.PtDirectParams(4, 16, 0, 0, 0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    b = H.PtDirectBuffers(lit=lit.ctypes.data_as(H._up))
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.pt_direct(None, C.byref(p), dp(P), dp(N), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_direct_device(None, C.byref(p), P.ctypes.data, N.ctypes.data, C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_direct_finish(None, None) == H.ERR_ARGUMENT
    assert np.all(lit == 7)


def test_every_refusal_of_the_parameter_block_is_an_argument_error_without_a_context(H):
    """pt_direct's checks run in the header's order and a NULL context is the first of them, so with no GPU every call below is PT_ERR_ARGUMENT for that reason
    alone; what pins each refusal of the parameter block here is pt_test_direct_host, which asks the very function pt_direct asks (tests/test_gpu_direct.py
    repeats them on a context). Nothing is written either way."""
    lib = H.lib()
    P, N, Lt = np.zeros((4, 3)), np.ones((4, 3)), np.ones(15)
    O, D, T, E = np.full((4, 3), 7.0), np.full((4, 1, 64, 3), 7.0), np.full((4, 1, 64), 7.0), np.full((4, 1, 64, 3), 7.0)
    valid, lit = np.full(4, 7, dtype=np.uint8), np.full(4, 7, dtype=np.uint32)
    dp = lambda a: a.ctypes.data_as(H._dp)
    hook = lambda p, *a: lib.pt_test_direct_host(4, C.byref(p) if p is not None else None, *a)
    full = (dp(P), dp(N), 1, dp(Lt), dp(O), dp(D), dp(T), dp(E), valid.ctypes.data_as(H._u8p))
    ok = dict(n=4, samples=16, pass_index=0, seed=0, first_index=0, bias=0.0, flags=0)
    bad = [dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=128), dict(bias=-1.0), dict(bias=float("inf")), dict(bias=float("nan")), dict(flags=4),
           dict(flags=H.AO_FACE_EYE | H.DIRECT_TO_LIGHT | 8)]
    for change in bad:
        p = H.PtDirectParams(**dict(ok, **change))
        assert hook(p, *full) == H.ERR_ARGUMENT, change
        assert lib.pt_direct(None, C.byref(p), dp(P), dp(N), C.byref(H.PtDirectBuffers(lit=lit.ctypes.data_as(H._up))), None) == H.ERR_ARGUMENT, change
    p = H.PtDirectParams(**dict(ok, flags=H.AO_FACE_EYE))
    p.eye[2] = float("inf")
    assert hook(p, *full) == H.ERR_ARGUMENT
    assert np.all(O == 7.0) and np.all(D == 7.0) and np.all(T == 7.0) and np.all(E == 7.0) and np.all(valid == 7) and np.all(lit == 7)
    p = H.PtDirectParams(**ok)
    for k in (0, 1, 3, 4, 5, 6, 7, 8):  # every pointer; `lights` may be NULL only with n_lights = 0
        args = list(full)
        args[k] = None
        assert hook(p, *args) == H.ERR_ARGUMENT, k
    assert hook(p, dp(P), dp(N), 0, None, dp(O), dp(D), dp(T), dp(E), valid.ctypes.data_as(H._u8p)) == H.OK
    assert np.all(O == 0.0) and np.all(valid == 1), "no lights: origins and valid are still written"


def test_the_refusals_stand_in_the_headers_order_in_front_of_the_first_hip_call():
    text = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_api.hip")).read()

    def body(signature):
        at = text.index(signature)
        return text[at:text.index("\n}\n", at)]
    check = body("static int pt_direct_check(")
    words = ["NULL context, params, positions, normals or buffers", "no output buffer asked for", "pt_direct_params_error(p)", "PT_ERR_NO_SCENE", "c->rays.pass.pending"]
    assert [check.index(w) for w in words] == sorted(check.index(w) for w in words)
    params = body("static const char* pt_direct_params_error(")
    words = ["more than PT_AO_MAX points", "samples must be a power of two", "bias must be finite and not negative", "unknown flags", "PT_AO_FACE_EYE needs a finite eye"]
    assert [params.index(w) for w in words] == sorted(params.index(w) for w in words)
    hip_call = re.compile(r"\bhip[A-Z]\w*\(|PT_HIP\(")
    assert "radius" not in params and not hip_call.search(check) and not hip_call.search(params), "pt_ao's list without the radius rule, and no HIP call"
    for signature in ('extern "C" int pt_direct(', 'extern "C" int pt_direct_device('):
        b = body(signature)
        assert b.index("pt_direct_check(") < b.index("p->n == 0") < b.index("hipSetDevice") < b.index("pt_direct_common("), signature
        assert not hip_call.search(b[:b.index("p->n == 0")]), "n = 0 is PT_OK before any HIP call"
    dev = body('extern "C" int pt_direct_device(')
    assert dev.count("pt_check_device_pointer(") == 5 and dev.rindex("pt_check_device_pointer(") < dev.index("pt_direct_common("), "every caller pointer, before anything is queued"
    assert 'extern "C" int pt_direct_finish(pt_context* c, double* kernel_ms) { return pt_rays_finish(c, kernel_ms); }' in text
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    sec = header[header.index("/* ---- Direct light"):header.index("#define PT_DIRECT_TO_LIGHT")]
    words = ["a NULL context", "no buffer asked for", "n > PT_AO_MAX", "samples not a", "bias negative", "flags other than", "non-finite eye", "PT_ERR_NO_SCENE"]
    assert [sec.index(w) for w in words] == sorted(sec.index(w) for w in words)


def test_the_kernel_header_restates_and_edits_no_existing_one():
    direct = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_direct.h")).read()
    assert '#include "pt_math.h"' in direct and "pt_ao.h" not in direct.split("#pragma once")[1] and "pt_shade.h" not in direct.split("#pragma once")[1]
    assert "fma(" not in direct and "__fma" not in direct
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^PASSES := .*\bdirect\b", makefile, flags=re.M) and "$(OBJDIR)/pt_direct_m$(m).o" in makefile


class _NoLibrary:
    @staticmethod
    def make():
        from portrayer_amd import host

        class NoLibrary(host.Renderer):
            def __init__(self):  # no scene, no context: any library call would fail on the null handle
                self._h = C.c_void_p()
                self.scene = None
        return NoLibrary()


def test_renderer_direct_rejects_bad_arguments_before_any_library_call():
    r = _NoLibrary.make()
    P, N = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="want"):
        r.direct(P, N, want=("sum", "bent"))
    with pytest.raises(ValueError, match="want"):
        r.direct(P, N, want=())
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.direct(P, N[:7])
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        r.direct(P.ravel(), N.ravel())
    with pytest.raises(ValueError, match="float64"):
        r.direct(P.astype(np.float32), N.astype(np.float32))
    for S in (0, 3, 128, 16.0, True, None):
        with pytest.raises(ValueError, match="samples"):
            r.direct(P, N, samples=S)
    for bias in (-1e-9, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="bias"):
            r.direct(P, N, bias=bias)
    for name in ("seed", "pass_index", "first_index"):
        for v in (-1, 1.5, True, 1 << 64):
            with pytest.raises(ValueError, match=name):
                r.direct(P, N, **{name: v})
    with pytest.raises(ValueError, match="pass_index"):
        r.direct(P, N, pass_index=1 << 32)
    for eye in ((0.0, 0.0), (0.0, float("nan"), 0.0), (0.0, 0.0, float("inf"))):
        with pytest.raises(ValueError, match="eye"):
            r.direct(P, N, eye=eye)
    for to_light in (1, None, "yes"):
        with pytest.raises(ValueError, match="to_light"):
            r.direct(P, N, to_light=to_light)
    with pytest.raises(ValueError, match="into"):
        r.direct(P, N, want=("lit",), into={"lit": np.zeros(8, dtype=np.int32)})
    with pytest.raises(ValueError, match="into"):
        r.direct(P, N, want=("sum",), into={"sum": np.zeros(8)})
    with pytest.raises(ValueError, match="into"):
        r.direct(P, N, want=("valid",), into={"valid": [0] * 8})


def test_renderer_direct_camera_and_chart_reject_bad_arguments_before_any_library_call():
    r = _NoLibrary.make()
    cam = np.zeros(10)
    for w, h in ((0, 8), (8, 0), (8.0, 8), (True, 8), (-1, 8)):
        with pytest.raises(ValueError, match="width|height"):
            r.direct_camera(cam, w, h)
        with pytest.raises(ValueError, match="width|height"):
            r.direct_chart(0, w, h)
    with pytest.raises(ValueError, match="points"):
        r.direct_camera(cam, 8192, 4096)  # 2^25 pixels > PT_AO_MAX
    with pytest.raises(ValueError, match="texels"):
        r.direct_chart(0, 8192, 4096)
    with pytest.raises(ValueError, match="samples"):
        r.direct_camera(cam, 8, 8, samples=5)
    with pytest.raises(ValueError, match="to_light"):
        r.direct_camera(cam, 8, 8, to_light=0)
    with pytest.raises(ValueError, match="into"):
        r.direct_camera(cam, 8, 4, want=("sum",), into={"sum": np.zeros((8, 4, 3))})
    with pytest.raises(ValueError, match="cam10"):
        r.direct_camera(np.zeros(9), 8, 8)
    with pytest.raises(ValueError, match="want"):
        r.direct_camera(cam, 8, 8, want=("mean",))
    with pytest.raises(ValueError, match="flip_normal"):
        r.direct_chart(0, 8, 8, flip_normal=1)
    with pytest.raises(ValueError, match="node"):
        r.direct_chart(-1, 8, 8)


def test_the_host_library_refuses_null_and_oversized_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    p = H.PtDirectParams(4, 16, 0, 0, 0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0))
    lit = np.zeros(4, dtype=np.uint32)
    b = H.PtDirectBuffers(lit=lit.ctypes.data_as(H._up))
    P = np.zeros((4, 3))
    cp = H.PtChartParams(0, 2, 2, 0)
    assert lib.ph_renderer_direct(None, C.byref(p), P.ctypes.data_as(H._dp), P.ctypes.data_as(H._dp), C.byref(b), None) == -1
    cam = np.zeros(10)
    assert lib.ph_renderer_direct_camera(None, cam.ctypes.data_as(H._dp), 2, 2, C.byref(p), C.byref(b), None) == -1
    assert lib.ph_renderer_direct_chart(None, C.byref(cp), None, C.byref(p), C.byref(b), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtDirectParams\s*\{[^}]*pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,\s*pub bias: f64, "
                     r"pub flags: u32, pub eye: \[f64; 3\],\s*\}", text)
    assert re.search(r"pub struct PtDirectBuffers\s*\{[^}]*pub sum: \*mut f64, pub lit: \*mut u32, pub valid: \*mut u8,\s*\}", text)
    for name in HIP_CALLS[:3]:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_direct\([^)]*params: \*const PtDirectParams, positions: \*const f64, normals: \*const f64, host_out: \*const PtDirectBuffers,", text)
    assert re.search(r"pub const PT_DIRECT_TO_LIGHT: u32 = 2;", text)
