"""The bounded-segment ray queries (pt_segments) without a GPU: argument checks that come before any HIP call, the declarations in the headers, the
libraries and the shim, and what Renderer.rays checks about `t_max` itself."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_every_argument_error_comes_before_any_hip_call(H):
    """No GPU and no context here: a NULL context, alone and together with every other argument error of the header - pt_rays' and the NULL t_max -,
    is PT_ERR_ARGUMENT; no call dereferences the context or reaches the runtime. (With a live context: tests/test_gpu_segments.py.)"""
    lib = H.lib()
    n = 4
    o, d, tm = np.zeros((n, 3)), np.ones((n, 3)), np.ones(n)
    t, occ = np.zeros(n), np.zeros(n, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    good_p = H.PtRaysParams(n, 0, 0)
    good_b = H.PtRaysBuffers(t=dp(t))
    occ_b = H.PtRaysBuffers(occluded=occ.ctypes.data_as(H._u8p))
    cases = [
        (good_p, dp(o), dp(d), dp(tm), good_b),                                   # only the context is NULL
        (None, dp(o), dp(d), dp(tm), good_b),                                     # params
        (good_p, None, dp(d), dp(tm), good_b), (good_p, dp(o), None, dp(tm), good_b),  # an input
        (good_p, dp(o), dp(d), None, good_b),                                     # the bounds
        (good_p, dp(o), dp(d), dp(tm), H.PtRaysBuffers()), (good_p, dp(o), dp(d), dp(tm), None),  # no buffer requested
        (H.PtRaysParams(H.RAYS_MAX + 1, 0, 0), dp(o), dp(d), dp(tm), good_b),     # n beyond the limit
        (H.PtRaysParams(n, 2, 0), dp(o), dp(d), dp(tm), occ_b), (H.PtRaysParams(n, -1, 0), dp(o), dp(d), dp(tm), occ_b),  # any_hit
        (H.PtRaysParams(n, 0, 2), dp(o), dp(d), dp(tm), good_b), (H.PtRaysParams(n, 0, -1), dp(o), dp(d), dp(tm), good_b),  # reorder
        (H.PtRaysParams(n, 1, 0), dp(o), dp(d), dp(tm), good_b),                  # an occlusion query asking for more than `occluded`
        (H.PtRaysParams(0, 0, 0), dp(o), dp(d), dp(tm), good_b),                  # n = 0 is fine only with a context
    ]
    for p, po, pd, pt, b in cases:
        pp = C.byref(p) if p is not None else None
        pb = C.byref(b) if b is not None else None
        assert lib.pt_segments(None, pp, po, pd, pt, pb, None) == H.ERR_ARGUMENT
        assert lib.pt_segments_device(None, pp, po, pd, pt, pb, None) == H.ERR_ARGUMENT
    assert not t.any() and not occ.any()


def test_the_abi_number_stays_and_pt_rays_params_did_not_grow(H):
    from __graft_entry__ import header_abi_version
    assert header_abi_version() == 8 and H.lib().pt_abi_version() == 8
    assert C.sizeof(H.PtRaysParams) == 16 and [n for n, _ in H.PtRaysParams._fields_] == ["n", "any_hit", "reorder"]
    assert not H.missing_symbols()


def test_headers_declare_the_pass_and_the_libraries_export_it(H):
    with open(os.path.join(ROOT, "include", "portrayer_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("pt_segments", "pt_segments_device"):
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in H.EXPORTS and hasattr(H.lib(), name), name
        assert getattr(H.lib(), name).argtypes is not None and len(getattr(H.lib(), name).argtypes) == 7, name
    with open(os.path.join(ROOT, "include", "portrayer_host.h")) as fh:
        assert re.search(r"\bint ph_renderer_segments\s*\(", re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S))
    from portrayer_amd import host
    assert "ph_renderer_segments" in host.EXPORTS and hasattr(host.lib(), "ph_renderer_segments")


def test_the_shim_declares_the_pass():
    ffi = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    for name in ("pt_segments", "pt_segments_device"):
        assert re.search(r"\bpub fn %s\s*\(" % name, ffi), name


def test_renderer_rays_takes_t_max_and_checks_it_before_any_library_call():
    from portrayer_amd import host

    sig = inspect.signature(host.Renderer.rays)
    assert "t_max" in sig.parameters and sig.parameters["t_max"].default is None

    class NoLibrary(host.Renderer):
        def __init__(self):  # no scene, no context: any library call would fail on the null handle
            self._h = C.c_void_p()
            self.scene = None

    r = NoLibrary()
    o, d = np.zeros((8, 3)), np.ones((8, 3))
    with pytest.raises(ValueError, match="t_max"):
        r.rays(o, d, t_max=np.ones(7))
    with pytest.raises(ValueError, match="t_max"):
        r.rays(o, d, t_max=np.ones((8, 1)))
    with pytest.raises(ValueError, match="t_max"):
        r.rays(o, d, t_max=np.ones(8, dtype=np.float32))
    with pytest.raises(ValueError, match="any_hit"):  # the unbounded pass's rules hold with a bound as well
        r.rays(o, d, any_hit=True, want=("t",), t_max=1.0)
