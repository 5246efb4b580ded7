"""The film's lens without a GPU: the header's declarations and both libraries' exports, the ctypes struct against the header's, every refusal that comes
before a HIP call, Lens' and Film.add's own argument checks, the Makefile's passes, and the declarations in INTEGRATION.md and the shim."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_CALLS = ("pt_film_add_lens", "pt_film_add_lens_device", "pt_test_lens_rays_host")
HOST_CALLS = ("ph_renderer_film_add_lens",)
LENS_FIELDS = ["model", "aperture", "focus", "extent"]


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_header_declares_the_calls_and_the_libraries_export_them(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HIP_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in H.EXPORTS and hasattr(H.lib(), name), name
    assert re.search(r"enum \{ PT_LENS_THIN = 0, PT_LENS_ORTHO = 1, PT_LENS_STEREO = 2 \};", text)
    assert (H.LENS_THIN, H.LENS_ORTHO, H.LENS_STEREO) == (0, 1, 2)
    assert not H.missing_symbols()
    from portrayer_amd import host
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in HOST_CALLS:
        assert re.search(r"\bint %s\s*\(" % name, text) and name in host.EXPORTS and hasattr(host.lib(), name), name


def test_the_additions_move_nothing_that_exists(H):
    assert H.lib().pt_abi_version() == 8
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        assert re.search(r"^#define PT_ABI_VERSION 8$", fh.read(), flags=re.M)
    assert C.sizeof(H.PtFilmParams) == 40 and C.sizeof(H.PtFilmMapParams) == 40 and C.sizeof(H.PtRadianceParams) == 40 and C.sizeof(H.PtCamera) == 184
    src = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_film_inst.h")).read()
    assert "lens" not in src.lower(), "PtFilmArgs and PtFilmSource stay as they are: the lens has an argument block and a source of its own"
    assert "lens" not in open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_film.h")).read().lower()


def test_the_ctypes_struct_has_the_headers_layout(H, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is part of the build (the oracle, tests/shim_replay.c)"
    lines = ['printf("lens %zu\\n", sizeof(pt_lens));'] + ['printf("l.%s %%zu\\n", offsetof(pt_lens, %s));' % (f, f) for f in LENS_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "portrayer_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["lens"]) == C.sizeof(H.PtLens) == 32
    assert [n for n, _ in H.PtLens._fields_] == LENS_FIELDS
    for f in LENS_FIELDS:
        assert int(got["l." + f]) == getattr(H.PtLens, f).offset, f
    # the kernel's copy of the four fields has the same shape
    dev = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_lens.h")).read()
    assert re.search(r"struct PtLensSet \{\s*int32_t model;\s*double aperture, focus, extent;\s*\};", dev)


def test_every_refusal_before_a_hip_call_is_an_argument_error_and_writes_nothing(H):
    """pt_film_add's checks come first and a NULL context is the first of them, so with no GPU every call below is PT_ERR_ARGUMENT; the refusals of the lens are
    repeated on a live context, where their own words can be read, by tests/test_gpu_lens.py, and through pt_test_lens_rays_host by tests/test_lens_contract.py."""
    lib = H.lib()
    cam, bg = H.PtCamera(), np.zeros((4, 4, 3))
    p = H.PtFilmParams(H.PtRect(0, 0, 3, 3), 1, 0, 0, 0)
    ms = C.c_double(7.0)
    dp = lambda a: a.ctypes.data_as(H._dp)
    for lens in (None, H.PtLens(0, 0.1, 1.0, 1.0), H.PtLens(5, 0.0, 1.0, 1.0), H.PtLens(0, -1.0, 1.0, 1.0)):
        lp = C.byref(lens) if lens is not None else None
        assert lib.pt_film_add_lens(None, None, C.byref(cam), lp, dp(bg), C.byref(p), C.byref(ms)) == H.ERR_ARGUMENT
        assert lib.pt_film_add_lens_device(None, None, C.byref(cam), lp, bg.ctypes.data, C.byref(p), None) == H.ERR_ARGUMENT
    assert ms.value == 7.0


def function_body(text, signature):
    start = text.index(signature)
    return text[start:text.index("\n}\n", start)]


def test_the_refusals_stand_in_the_source_in_the_headers_order_before_the_first_hip_call():
    """What a machine without a GPU can say about the refusals of a LIVE context: pt_film_add's list (pt_film_add_check) is asked first, then pt_lens_check,
    which holds the lens' refusals in the order the header lists them; neither calls anything of HIP, and both entry points go through them before anything else."""
    api = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_api.hip")).read()
    check = function_body(api, "static int pt_lens_check(")
    assert "hip" not in check and "PT_HIP" not in check
    order = ["NULL lens", "unknown lens model", "aperture must be finite and not negative", "focus must be finite and positive", "extent must be finite and positive"]
    at = [check.index(w) for w in order]
    assert at == sorted(at)
    assert check.count("PT_ERR_ARGUMENT") == len(order)
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    errors = header[header.index("all of pt_film_add's, in its order, then PT_ERR_ARGUMENT for a NULL lens"):]
    words = ["NULL lens", "unknown model", "aperture not finite or < 0", "focus not finite or <= 0", "extent not finite or <= 0"]
    at = [errors.index(w) for w in words]
    assert at == sorted(at)
    film_check = function_body(api, "static int pt_film_add_check(")
    assert "hip" not in film_check and "PT_HIP" not in film_check
    for shared in ("static int pt_film_add_host(", "static int pt_film_add_queued("):
        body = function_body(api, shared)
        assert body.index("pt_film_add_check(") < body.index("pt_lens_check(") < body.index("pt_film_slice_empty(p)) return PT_OK") < body.index("PT_HIP(")
        assert "lens, " in body[body.index("pt_film_add_common("):]
    # the four entry points share everything but the launcher: one body for the host path, one for the queued path, one common queue
    for entry, shared in (('extern "C" int pt_film_add(', "pt_film_add_host(c, f, cam, nullptr, false,"), ('extern "C" int pt_film_add_lens(', "pt_film_add_host(c, f, cam, lens, true,"),
                          ('extern "C" int pt_film_add_device(', "pt_film_add_queued(c, f, cam, nullptr, false,"),
                          ('extern "C" int pt_film_add_lens_device(', "pt_film_add_queued(c, f, cam, lens, true,")):
        body = function_body(api, entry)
        assert shared in body and "PT_HIP" not in body and body.count(";") == 1, entry
    common = function_body(api, "static int pt_film_add_common(")
    assert common.count("pt_film_dispatch(") == 1 and common.count("pt_lens_dispatch(") == 1 and common.count("pt_film_fold_launch(") == 1 and common.count("pt_film_fold_map_launch(") == 1


def test_the_makefile_builds_the_pass_per_mode_and_the_compare_tool_knows_it():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    passes = re.search(r"^PASSES := (.*)$", mk, flags=re.M).group(1).split()
    assert "lens" in passes and "$(foreach m,$(RENDER_MODES),$(OBJDIR)/pt_lens_m$(m).o)" in mk
    tool = open(os.path.join(ROOT, "tools", "compare_render_objects.py")).read()
    assert tuple(passes) == eval(re.search(r"^PASSES = (\(.*\))$", tool, flags=re.M).group(1))
    for f in ("pt_lens.h", "pt_lens_inst.h", "pt_lens_inst.hip"):
        assert os.path.exists(os.path.join(ROOT, "portrayer_amd", "csrc", f)), f
    contract = open(os.path.join(ROOT, "portrayer_amd", "csrc", "pt_lens.h")).read()
    code = re.sub(r"//.*", "", contract)
    assert not re.search(r"\b(sin|cos|tan|atan2|acos|pow|exp|log|fma)\s*\(", code), "no libm call and no fused operation in the contract"
    assert '#include "pt_ao_tables.h"' in contract and "_tables.h" not in contract.replace("pt_ao_tables.h", ""), "no new table"


def test_lens_rejects_bad_arguments_before_any_library_call():
    from portrayer_amd import host
    nan, inf = float("nan"), float("inf")
    for a in (-1e-9, nan, inf, None, True, "1"):
        with pytest.raises(ValueError, match="aperture"):
            host.Lens.thin(a, 1.0)
    for f in (0.0, -1.0, nan, inf, None, True):
        with pytest.raises(ValueError, match="focus"):
            host.Lens.thin(0.1, f)
    for e in (0.0, -2.0, nan, inf, None, False):
        with pytest.raises(ValueError, match="half_height"):
            host.Lens.ortho(e)
    for fov in (0.0, -10.0, 360.0, 400.0, nan, inf, None):
        with pytest.raises(ValueError, match="fov_degrees"):
            host.Lens.fisheye(fov)
    thin, ortho, eye = host.Lens.thin(0, 2), host.Lens.ortho(1.5), host.Lens.fisheye(180.0)
    assert (thin.model, thin.aperture, thin.focus) == (0, 0.0, 2.0) and (ortho.model, ortho.extent) == (1, 1.5)
    assert eye.model == 2 and eye.extent == np.tan(np.pi / 4.0)
    s = thin.struct()
    assert (s.model, s.aperture, s.focus) == (0, 0.0, 2.0)
    for model in (3, -1, None, True):
        with pytest.raises(ValueError, match="model"):
            host.Lens(model).struct()
    broken = host.Lens.ortho(1.0)
    broken.extent = nan
    with pytest.raises(ValueError, match="extent"):
        broken.struct()


def test_film_add_rejects_a_bad_lens_before_any_library_call():
    from portrayer_amd import host

    class NoLibrary(host.Film):
        """A film with no renderer and no handle: any library call would fail on them."""
        def __init__(self):
            self._h, self._r = C.c_void_p(), None
            self.width, self.height, self.moments = 4, 4, False

    film = NoLibrary()
    cam, bg = np.zeros(10), np.zeros((4, 4, 3))
    for lens in (1, "thin", (0, 0.1, 1.0, 1.0), host.H.PtLens(0, 0.1, 1.0, 1.0)):
        with pytest.raises(ValueError, match="lens"):
            film.add(cam, bg, lens=lens)
    broken = host.Lens.thin(0.1, 1.0)
    broken.focus = 0.0
    with pytest.raises(ValueError, match="focus"):
        film.add(cam, bg, lens=broken)
    with pytest.raises(ValueError, match="samples"):
        film.add(cam, bg, samples=0, lens=host.Lens.ortho(1.0))
    assert "supply your own `guides=`" in host.Film.denoise.__doc__ and "PINHOLE" in host.Film.denoise.__doc__


def test_the_host_library_refuses_null_calls_before_the_device_library(H):
    from portrayer_amd import host
    lib = host.lib()
    p = H.PtFilmParams(H.PtRect(0, 0, 3, 3), 1, 0, 0, 0)
    lens, cam, bg = H.PtLens(0, 0.0, 1.0, 1.0), np.zeros(10), np.zeros((4, 4, 3))
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.ph_renderer_film_add_lens(None, None, dp(cam), C.byref(lens), dp(bg), C.byref(p), None) == -1


@pytest.mark.parametrize("path", ["INTEGRATION.md", os.path.join("shim", "src", "hip_ffi.rs")])
def test_the_integration_guide_and_the_shim_declare_the_calls(path):
    text = open(os.path.join(ROOT, path)).read()
    assert re.search(r"#\[repr\(C\)\]\s*pub struct PtLens\s*\{[^}]*pub model: i32, pub aperture: f64, pub focus: f64, pub extent: f64,\s*\}", text)
    assert re.search(r"pub fn pt_film_add_lens\(ctx: \*mut PtContext, film: \*mut PtFilm, camera: \*const PtCamera, lens: \*const PtLens, background: \*const f64,\s*"
                     r"params: \*const PtFilmParams, kernel_ms: \*mut f64\) -> c_int;", text)
    assert re.search(r"pub fn pt_film_add_lens_device\(ctx: \*mut PtContext, film: \*mut PtFilm, camera: \*const PtCamera, lens: \*const PtLens, d_background: \*const f64,\s*"
                     r"params: \*const PtFilmParams, hip_stream: \*mut c_void\) -> c_int;", text)
