"""pt_vertex_bounds_device / pt_scene_deform_device / Renderer.deform_device: what can be checked without a GPU - the exports, the struct's layout, the
bindings, the refusal of a NULL context, and the argument checks of Renderer.deform_device, which raise before any library call (a stub stands in for the
library)."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_libraries_export_the_new_entry_points():
    from portrayer_amd import _hip, host
    for name in ("pt_vertex_bounds_device", "pt_scene_deform_device", "pt_test_vertex_box_shape"):
        assert hasattr(_hip.lib(), name), name
        assert name in _hip.EXPORTS and name in _hip.header_functions()
    for name in ("ph_renderer_deform_device", "ph_renderer_mesh_count", "ph_renderer_mesh_vertices"):
        assert hasattr(host.lib(), name), name
        assert name in host.EXPORTS
    assert _hip.missing_symbols() == []
    assert _hip.lib().pt_abi_version() == 8


def test_the_ctypes_struct_has_the_headers_fields_in_order():
    from portrayer_amd import _hip
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pt_mesh_deform_device;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _hip.PtMeshDeformDevice._fields_] == ["mesh", "d_positions", "d_normals", "bounds_invtrans", "rebuild"]
    # 4 + pad, 3 x 8, 4 + pad: pt_mesh_deform's layout
    assert C.sizeof(_hip.PtMeshDeformDevice) == C.sizeof(_hip.PtMeshDeform) == 8 + 24 + 8
    for mine, theirs in zip(_hip.PtMeshDeformDevice._fields_, _hip.PtMeshDeform._fields_):
        assert getattr(_hip.PtMeshDeformDevice, mine[0]).offset == getattr(_hip.PtMeshDeform, theirs[0]).offset


def test_the_host_struct_has_the_headers_fields_in_order():
    from portrayer_amd import host
    header = open(os.path.join(ROOT, "include", "portrayer_host.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ph_device_mesh;", header).group(1)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in host.PhDeviceMesh._fields_] == ["mesh", "d_positions", "d_normals"]
    assert C.sizeof(host.PhDeviceMesh) == 24


def test_the_rust_declarations_are_in_step_with_the_header():
    text = open(os.path.join(ROOT, "shim", "src", "hip_ffi.rs")).read()
    body = re.search(r"pub struct PtMeshDeformDevice \{(.*?)\n\}", text, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", body) == ["mesh", "d_positions", "d_normals", "bounds_invtrans", "rebuild"]
    assert "pub fn pt_vertex_bounds_device(" in text and "pub fn pt_scene_deform_device(" in text


def test_the_python_bindings_exist():
    from portrayer_amd import _hip, host
    assert callable(host.Renderer.deform_device) and callable(host.Renderer.mesh_vertices) and callable(host.Renderer.mesh_count)
    assert callable(_hip.Context.deform_device) and callable(_hip.Context.vertex_bounds_device)


def test_a_null_context_is_refused_without_a_device():
    from portrayer_amd import _hip, host
    mo, df = _hip.PtSceneMotion(), _hip.PtMeshDeformDevice()
    box, bad = np.zeros(6), C.c_uint64(0)
    L = _hip.lib()
    assert L.pt_scene_deform_device(None, 1, C.byref(df), C.byref(mo), None) == -1  # PT_ERR_ARGUMENT
    assert L.pt_scene_deform_device(None, 0, None, C.byref(mo), None) == -1
    assert L.pt_vertex_bounds_device(None, 0, None, _hip._p(box, _hip._dp), C.byref(bad)) == -1
    assert L.pt_vertex_bounds_device(None, 3, None, _hip._p(box, _hip._dp), C.byref(bad)) == -1
    assert L.pt_test_vertex_box_shape(None, None) == -1
    assert host.lib().ph_renderer_deform_device(None, 0, None, 0, None) == -1
    assert host.lib().ph_renderer_mesh_count(None) == -1 and host.lib().ph_renderer_mesh_vertices(None, 0) == -1


class _Stub:
    """what Renderer.deform_device asks of the host library, with the deform call counted instead of made"""

    def __init__(self, vertices):
        self.vertices, self.calls = vertices, 0

    def ph_renderer_mesh_count(self, h):
        return len(self.vertices)

    def ph_renderer_mesh_vertices(self, h, m):
        return self.vertices[m]

    def ph_renderer_deform_device(self, *a):
        self.calls += 1
        return 0

    def ph_renderer_destroy(self, h):
        pass


@pytest.fixture
def stubbed(monkeypatch):
    from portrayer_amd import host
    stub = _Stub([5, 7])
    monkeypatch.setattr(host, "lib", lambda: stub)
    r = host.Renderer.__new__(host.Renderer)
    r._h, r.scene, r._device = C.c_void_p(), None, 0
    return r, stub


def _fake_device_tensor(t, index=0):
    """a CPU tensor that says it lives on cuda:<index>: the checks behind the device check can be reached without a GPU"""
    class OnDevice(torch.Tensor):
        @property
        def device(self):
            return types.SimpleNamespace(type="cuda", index=index)
    return t.as_subclass(OnDevice)


BAD = {
    "float32": lambda: torch.zeros((5, 3), dtype=torch.float32),
    "one vertex too few": lambda: torch.zeros((4, 3), dtype=torch.float64),
    "one vertex too many": lambda: torch.zeros((6, 3), dtype=torch.float64),
    "flat": lambda: torch.zeros(15, dtype=torch.float64),
    "four columns": lambda: torch.zeros((5, 4), dtype=torch.float64),
    "not contiguous": lambda: torch.zeros((3, 5), dtype=torch.float64).t(),
    "strided": lambda: torch.zeros((5, 6), dtype=torch.float64)[:, ::2],
    "a numpy array": lambda: np.zeros((5, 3)),
}


@pytest.mark.parametrize("what", list(BAD))
def test_deform_device_checks_the_tensor_before_any_library_call(stubbed, what):
    r, stub = stubbed
    t = BAD[what]()
    if isinstance(t, torch.Tensor):
        assert what != "not contiguous" or (tuple(t.shape) == (5, 3) and not t.is_contiguous())
        t = _fake_device_tensor(t)  # (so that it is the property under test that fails, not the device check)
    with pytest.raises(ValueError):
        r.deform_device({0: t})
    good = _fake_device_tensor(torch.zeros((5, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        r.deform_device({0: good}, normals={0: t})
    assert stub.calls == 0


def test_deform_device_refuses_a_cpu_tensor_and_another_device(stubbed):
    r, stub = stubbed
    cpu = torch.zeros((5, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="deform\\(\\) for host data"):
        r.deform_device({0: cpu})
    with pytest.raises(ValueError, match="the renderer is on cuda:0"):
        r.deform_device({0: _fake_device_tensor(cpu, index=1)})
    assert stub.calls == 0


def test_deform_device_checks_the_mesh_indices_and_the_dicts(stubbed):
    r, stub = stubbed
    good = _fake_device_tensor(torch.zeros((5, 3), dtype=torch.float64))
    for bad in (2, -1, "0", True, 0.0):
        with pytest.raises(ValueError):
            r.deform_device({bad: good})
    with pytest.raises(ValueError):
        r.deform_device({0: good}, normals={1: _fake_device_tensor(torch.zeros((7, 3), dtype=torch.float64))})  # normals without positions
    with pytest.raises(ValueError):
        r.deform_device([good])
    with pytest.raises(ValueError):
        r.mesh_vertices(2)
    assert stub.calls == 0 and r.mesh_vertices(1) == 7


def test_a_good_call_reaches_the_library_once(stubbed):
    r, stub = stubbed
    r.deform_device({0: _fake_device_tensor(torch.zeros((5, 3), dtype=torch.float64)), 1: _fake_device_tensor(torch.zeros((7, 3), dtype=torch.float64))},
                    normals={1: _fake_device_tensor(torch.zeros((7, 3), dtype=torch.float64))}, rebuild=True)
    assert stub.calls == 1
