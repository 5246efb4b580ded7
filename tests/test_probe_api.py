"""The probe pass without a GPU: the header's declarations and both libraries' exports, the ctypes structs against the header's, every refusal that comes before
a HIP call, Renderer.probe's and Renderer.probe_grid's own argument checks, host.sh_irradiance, the Makefile's passes, and the declarations in INTEGRATION.md
and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_probe", "pt_probe_device", "pt_probe_finish", "pt_test_probe_host", "pt_test_probe_tables")
HOST_CALLS = ("ph_renderer_probe",)
PARAM_FIELDS = ["n", "samples", "pass", "seed", "first_index"]  # the header's names; ctypes says pass_index (`pass` is a keyword)
BUFFER_FIELDS = ["sh", "valid"]


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
    assert C.sizeof(H.PtAoParams) == 80 and C.sizeof(H.PtGatherParams) == 72 and C.sizeof(H.PtRadianceParams) == 40
    assert H.PROBE_MAX == 1 << 20 == H.RAYS_MAX // 1024 and H.PROBE_SAMPLES == (64, 128, 256, 512, 1024)
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        assert re.search(r"#define PT_PROBE_MAX \(PT_RAYS_MAX / 1024\)", fh.read())


def test_ctypes_structs_have_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("params %zu\\n", sizeof(pt_probe_params));', 'printf("buffers %zu\\n", sizeof(pt_probe_buffers));', 'printf("max %llu\\n", (unsigned long long)PT_PROBE_MAX);']
    lines += ['printf("p.%s %%zu\\n", offsetof(pt_probe_params, %s));' % (f, f) for f in PARAM_FIELDS]
    lines += ['printf("b.%s %%zu\\n", offsetof(pt_probe_buffers, %s));' % (f, f) for f in BUFFER_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["params"]) == C.sizeof(H.PtProbeParams) == 32 and int(got["buffers"]) == C.sizeof(H.PtProbeBuffers) == 16 and int(got["max"]) == H.PROBE_MAX
    assert [n for n, _ in H.PtProbeParams._fields_] == [f if f != "pass" else "pass_index" for f in PARAM_FIELDS]
    assert [n for n, _ in H.PtProbeBuffers._fields_] == BUFFER_FIELDS == list(H.PROBE_BUFFERS)
    for f in PARAM_FIELDS:
        assert int(got["p." + f]) == getattr(H.PtProbeParams, f if f != "pass" else "pass_index").offset, f
    for f in BUFFER_FIELDS:
        assert int(got["b." + f]) == getattr(H.PtProbeBuffers, f).offset, f


def test_every_refusal_before_a_hip_call_is_an_argument_error_and_writes_nothing(H):
    """pt_probe's checks run in the header's order and a NULL context is the first of them, so with no GPU every call below is PT_ERR_ARGUMENT; the refusals of
    the parameter block are repeated on a live context, where their own words can be read, by tests/test_gpu_probe.py. Nothing is written either way."""
    lib = H.lib()
    P, bg = np.zeros((4, 3)), np.array([0.25, 0.5, 1.0])
    sh, valid = np.full((4, 9, 3), 7.0), np.full(4, 7, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ok = dict(n=4, samples=64, pass_index=0, seed=0, first_index=0)
    b = H.PtProbeBuffers(sh=dp(sh), valid=valid.ctypes.data_as(H._u8p))
    p = H.PtProbeParams(**ok)
    assert lib.pt_probe(None, C.byref(p), dp(P), dp(bg), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_probe_device(None, C.byref(p), P.ctypes.data, dp(bg), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_probe_finish(None, None) == H.ERR_ARGUMENT
    for change in (dict(n=H.PROBE_MAX + 1), dict(samples=0), dict(samples=16), dict(samples=65), dict(samples=192), dict(samples=2048)):
        q = H.PtProbeParams(**dict(ok, **change))
        assert lib.pt_probe(None, C.byref(q), dp(P), dp(bg), C.byref(b), None) == H.ERR_ARGUMENT, change
        assert lib.pt_probe_device(None, C.byref(q), P.ctypes.data, dp(bg), C.byref(b), None) == H.ERR_ARGUMENT, change
    for args in ((None, dp(P), dp(bg), C.byref(b)), (C.byref(p), None, dp(bg), C.byref(b)), (C.byref(p), dp(P), None, C.byref(b)), (C.byref(p), dp(P), dp(bg), None),
                 (C.byref(p), dp(P), dp(bg), C.byref(H.PtProbeBuffers()))):
        assert lib.pt_probe(None, *args, None) == H.ERR_ARGUMENT
    assert np.all(sh == 7.0) and np.all(valid == 7)


def test_the_refusals_stand_in_the_source_in_the_headers_order_before_the_first_hip_call():
    """What a machine without a GPU can say about the refusals of a LIVE context: pt_probe_check holds every one of them, in the order the header lists them,
    calls nothing of HIP, and both entry points ask it before anything else."""
    api = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_api.hip")).read()
    start = api.index("static int pt_probe_check(")
    check = api[start:api.index("\n}\n", start)]
    assert "hip" not in check.replace("hip_stream", "") and "PT_HIP" not in check
    order = ["NULL context, params, positions, background or buffers", "no output buffer asked for", "more than PT_PROBE_MAX probes", "samples must be 64, 128, 256, 512 or 1024",
             "PT_ERR_NO_SCENE", "c->radiance.pass.pending"]
    at = [check.index(w) for w in order]
    assert at == sorted(at)
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    errors = header[header.index("a NULL context / params / positions / background / buffers; no buffer asked for; n > PT_PROBE_MAX; samples"):]
    assert errors.index("samples") < errors.index("PT_ERR_NO_SCENE") < errors.index("n = 0 is PT_OK")
    for entry in ('extern "C" int pt_probe(', 'extern "C" int pt_probe_device('):
        s = api.index(entry)
        body = api[s:api.index("\n}\n", s)]
        assert body.index("pt_probe_check(") < body.index("PT_HIP(") and body.index("p->n == 0) return PT_OK") < body.index("PT_HIP(")
    assert 'extern "C" int pt_probe_finish(pt_context* c, double* kernel_ms) { return pt_radiance_finish(c, kernel_ms); }' in api
    common = api[api.index("static int pt_probe_common("):]
    common = common[:common.index("\n}\n")]
    assert "PT_PROBE_SCRATCH_BYTES ((size_t)32 << 20)" in api and "pt_probe_scratch_bound()" in common, "the partial sums are bounded at 32 MiB"
    assert common.index("pt_pass_open(") < common.index("hipMemsetAsync((char*)v.misc.p + 256, 0, PT_PASS_MISC_BYTES - 256, stream)") < common.index("pt_pass_seal("), \
        "several launches inside the one open pass, the queues zeroed in between as pt_film_add_common does"


def test_the_makefile_builds_the_pass_per_mode_and_the_compare_tool_knows_it():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    passes = re.search(r"^PASSES := (.*)$", mk, flags=re.M).group(1).split()
    assert "probe" in passes and "$(OBJDIR)/pt_probe.o $(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_probe_m$(m).o)" in mk
    tool = open(os.path.join(ROOT, "tools", "compare_render_objects.py")).read()
    assert tuple(passes) == eval(re.search(r"^PASSES = (\(.*\))$", tool, flags=re.M).group(1)) and '"pt_probe.o"' in tool
    for f in ("pt_probe.h", "pt_probe_tables.h", "pt_probe_inst.h", "pt_probe_inst.hip", "pt_probe.hip"):
        assert os.path.exists(os.path.join(ROOT, "portrayer_amd", "csrc", f)), f
    untouched = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_ao.h")).read()
    assert "probe" not in untouched.lower(), "pt_ao.h stays as it is: the probe contract restates the few lines"


def _NoLibrary():
    """A Renderer with no scene and no context: any library call would fail on the null handle."""
    from portrayer_amd import host

    class NoLibrary(host.Renderer):
        def __init__(self):
            self._h = C.c_void_p()
            self.scene = None
    return NoLibrary()


def test_renderer_probe_rejects_bad_arguments_before_any_library_call():
    r = _NoLibrary()
    P = np.zeros((8, 3))
    for want in (("sh", "coeffs"), (), "sh", ("sum",)):
        with pytest.raises(ValueError, match="want"):
            r.probe(P, want=want)
    for bad in (P.ravel(), np.zeros((8, 2)), np.zeros((2, 4, 3))):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            r.probe(bad)
    with pytest.raises(ValueError, match="float64"):
        r.probe(P.astype(np.float32))
    for S in (0, 16, 32, 96, 2048, 64.0, True, None):
        with pytest.raises(ValueError, match="samples"):
            r.probe(P, samples=S)
    for name in ("seed", "pass_index", "first_index"):
        for v in (-1, 1.5, True, 1 << 64):
            with pytest.raises(ValueError, match=name):
                r.probe(P, **{name: v})
    with pytest.raises(ValueError, match="pass_index"):
        r.probe(P, pass_index=1 << 32)
    for bg in ((0.0, 0.0), np.zeros((8, 3)), 1.0, "sky"):
        with pytest.raises(ValueError, match="background"):
            r.probe(P, background=bg)
    with pytest.raises(ValueError, match="into"):
        r.probe(P, into={"sh": np.zeros((8, 9, 3), dtype=np.float32)})
    with pytest.raises(ValueError, match="into"):
        r.probe(P, into={"sh": np.zeros((8, 27))})
    with pytest.raises(ValueError, match="into"):
        r.probe(P, want=("valid",), into={"valid": [0] * 8})
    with pytest.raises(ValueError, match="into"):
        r.probe(P, into=[np.zeros((8, 9, 3))])
    with pytest.raises(TypeError):
        r.probe(P, np.ones((8, 3)), normals=np.ones((8, 3)))  # a probe has no normal: there is no such argument


def test_probe_grid_checks_its_arguments_and_orders_its_points_x_slowest():
    r = _NoLibrary()
    for lo, hi in (((0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), 1.0)):
        with pytest.raises(ValueError, match="lo and hi"):
            r.probe_grid(lo, hi, (2, 2, 2))
    for shape in ((2, 2), (2, 2, 0), (2, 2.0, 2), (True, 2, 2), 8):
        with pytest.raises(ValueError, match="shape"):
            r.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), shape)
    with pytest.raises(ValueError, match="samples"):
        r.probe_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2), samples=100)

    seen = {}

    class Recorder(type(r)):
        def probe(self, points, background=(0.0, 0.0, 0.0), samples=256, seed=0, pass_index=0, first_index=0, want=("sh",), into=None):
            seen.update(points=points, samples=samples, seed=seed, pass_index=pass_index, first_index=first_index, want=want)
            n = len(points)
            return {"sh": np.arange(n * 27, dtype=np.float64).reshape(n, 9, 3), "coeffs": np.zeros((n, 9, 3)), "valid": np.arange(n, dtype=np.uint8), "kernel_ms": 1.5}

    g = Recorder().probe_grid((-1.0, 0.0, 10.0), (1.0, 3.0, 10.5), (3, 4, 2), samples=64, seed=5, pass_index=2, first_index=100, want=("sh", "valid"))
    pts = seen["points"]
    assert pts.shape == (24, 3) and pts.dtype == np.float64 and pts.flags.c_contiguous
    assert (seen["samples"], seen["seed"], seen["pass_index"], seen["first_index"], seen["want"]) == (64, 5, 2, 100, ("sh", "valid"))
    for i in range(3):
        for j in range(4):
            for k in range(2):
                assert list(pts[(i * 4 + j) * 2 + k]) == [-1.0 + i, float(j), 10.0 + 0.5 * k], "probe (i, j, k) is point (i * ny + j) * nz + k"
    assert g["sh"].shape == (3, 4, 2, 9, 3) and g["coeffs"].shape == (3, 4, 2, 9, 3) and g["valid"].shape == (3, 4, 2) and g["points"].shape == (3, 4, 2, 3)
    assert g["valid"][2, 1, 1] == (2 * 4 + 1) * 2 + 1 and g["sh"][1, 2, 0, 0, 0] == ((1 * 4 + 2) * 2) * 27 and g["kernel_ms"] == 1.5
    one = Recorder().probe_grid((1.0, 2.0, 3.0), (4.0, 5.0, 6.0), (1, 1, 2))
    assert np.array_equal(one["points"].reshape(-1, 3), [[1.0, 2.0, 3.0], [1.0, 2.0, 6.0]]), "an axis of one point sits at lo"


def test_sh_irradiance_of_a_constant_radiance_is_pi_times_it_for_any_normal():
    from portrayer_amd import host
    L = np.array([0.25, 1.0, 3.5])
    coeffs = np.zeros((9, 3))
    coeffs[0] = 2.0 * np.sqrt(np.pi) * L  # the integral of L Y00 over the sphere; every other coefficient of a constant is zero
    rng = np.random.default_rng(3)
    n = rng.normal(size=(500, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    n = np.vstack([n, np.eye(3), -np.eye(3)])
    E = host.sh_irradiance(coeffs, n)
    assert E.shape == (506, 3) and np.abs(E - np.pi * L[None, :]).max() <= 1e-12
    assert np.abs(host.sh_irradiance(coeffs, (0.0, 0.0, 1.0)) - np.pi * L).max() <= 1e-12


def test_sh_irradiance_applies_the_cosine_lobe_per_band_and_broadcasts():
    """The light of a distant lamp in direction w, L(d) = sum of Y_i(w) Y_i(d) up to order 2, lights a surface with E(n) = sum A_l Y_i(w) Y_i(n): checked
    against the closed form of each band (addition theorem): pi / (4 pi) + (2 pi / 3) (3 / (4 pi)) cos + (pi / 4) (5 / (4 pi)) P2(cos)."""
    from portrayer_amd import host
    rng = np.random.default_rng(4)
    w = rng.normal(size=3); w /= np.linalg.norm(w)
    n = rng.normal(size=(6, 7, 3)); n /= np.linalg.norm(n, axis=-1)[..., None]
    Y = host.sh_basis(w)
    assert Y.shape == (9,) and host.sh_basis(n).shape == (6, 7, 9)
    coeffs = np.repeat(Y[:, None], 3, axis=1) * np.array([1.0, 2.0, 0.5])
    E = host.sh_irradiance(coeffs, n)
    cos = n @ w
    want = 0.25 + 0.5 * cos + (5.0 / 16.0) * 0.5 * (3.0 * cos * cos - 1.0)
    assert E.shape == (6, 7, 3) and np.abs(E - want[..., None] * np.array([1.0, 2.0, 0.5])).max() <= 1e-12
    grid = host.sh_irradiance(np.broadcast_to(coeffs, (6, 7, 9, 3)), n[0, 0])  # a grid of probes, one normal
    assert grid.shape == (6, 7, 3) and np.abs(grid - E[0, 0]).max() <= 1e-15
    for bad in (np.zeros((9,)), np.zeros((3, 9)), np.zeros((4, 3))):
        with pytest.raises(ValueError, match="coeffs"):
            host.sh_irradiance(bad, n)
    with pytest.raises(ValueError, match="directions"):
        host.sh_irradiance(coeffs, np.zeros((5, 2)))


def test_the_docstrings_say_how_the_sums_become_coefficients():
    from portrayer_amd import host
    assert re.search(r"`coeffs` = sh \* 4 pi / samples", host.Renderer.probe.__doc__)
    assert "x slowest and z fastest" in host.Renderer.probe_grid.__doc__


def test_the_host_library_refuses_null_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    p = H.PtProbeParams(4, 64, 0, 0, 0)
    sh = np.zeros((4, 9, 3))
    b = H.PtProbeBuffers(sh=sh.ctypes.data_as(H._dp))
    P, bg = np.zeros((4, 3)), np.zeros(3)
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.ph_renderer_probe(None, C.byref(p), dp(P), dp(bg), C.byref(b), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"pub struct PtProbeParams\s*\{[^}]*pub n: u64, pub samples: u32, pub pass: u32, pub seed: u64, pub first_index: u64,\s*\}", text)
    assert re.search(r"pub struct PtProbeBuffers\s*\{[^}]*pub sh: \*mut f64, pub valid: \*mut u8,\s*\}", text)
    assert re.search(r"pub const PT_PROBE_MAX: u64 = 1 << 20;", text)
    for name in HIP_CALLS[:3]:
        assert re.search(r"pub fn %s\(" % name, text), name
    assert re.search(r"pub fn pt_probe\([^)]*params: \*const PtProbeParams, positions: \*const f64, background: \*const f64,\s*host_out: \*const PtProbeBuffers,", text)
    assert re.search(r"pub fn pt_probe_device\([^)]*d_positions: \*const f64, background: \*const f64,\s*device_out: \*const PtProbeBuffers, hip_stream: \*mut c_void\)", text)
