"""pt_scene_deform / Renderer.deform: what can be checked without a GPU - the exports, the struct's layout, the bindings, the topology check of
Scene.same_topology (a mesh may be bent, not re-meshed) and the argument check that needs no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import Light, Material, MeshData, Mesh, Node, Scene, Sphere, Texture  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_libraries_export_the_deform_entry_points():
    from portrayer_amd import _hip, host
    for name in ("pt_scene_deform", "pt_node_scene_deform", "pt_scene_mesh_rebuildable"):
        assert hasattr(_hip.lib(), name), name
        assert name in _hip.EXPORTS and name in _hip.header_functions()
    for name in ("ph_renderer_deform", "ph_scene_same_topology"):
        assert hasattr(host.lib(), name), name
        assert name in host.EXPORTS
    assert _hip.lib().pt_abi_version() == 8


def test_the_ctypes_struct_has_the_headers_fields_in_order():
    from portrayer_amd import _hip
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pt_mesh_deform;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in _hip.PtMeshDeform._fields_] == ["mesh", "positions", "normals", "bounds_invtrans", "rebuild"]
    # 4 + pad, 3 x 8, 4 + pad
    assert C.sizeof(_hip.PtMeshDeform) == 8 + 24 + 8
    assert _hip.PtMeshDeform.positions.offset == 8 and _hip.PtMeshDeform.bounds_invtrans.offset == 24 and _hip.PtMeshDeform.rebuild.offset == 32


def test_the_python_bindings_exist():
    from portrayer_amd import _hip, host
    assert callable(host.Renderer.deform) and callable(host.Scene.same_topology) and callable(_hip.Context.deform)


def test_a_null_context_is_refused_without_a_device():
    from portrayer_amd import _hip
    mo, df = _hip.PtSceneMotion(), _hip.PtMeshDeform()
    assert _hip.lib().pt_scene_deform(None, 1, C.byref(df), C.byref(mo), None) == -1  # PT_ERR_ARGUMENT
    assert _hip.lib().pt_scene_deform(None, 0, None, C.byref(mo), None) == -1
    assert _hip.lib().pt_node_scene_deform(None, 1, C.byref(df), C.byref(mo), None) == -1
    assert _hip.lib().pt_scene_mesh_rebuildable(None, 0) == -1


def sheet(n=3, phase=0.0, extra_vertex=False, flip=False, uv=None, normals=False):
    xs = np.linspace(-1.0, 1.0, n + 1)
    pos = np.array([[x, y, 0.3 * np.sin(2.0 * x + phase)] for y in xs for x in xs], dtype=np.float64)
    tris = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            tris += [[a, a + 1, a + n + 2], [a, a + n + 2, a + n + 1]]
    tris = np.array(tris, dtype=np.uint32)
    if flip:
        tris[0] = tris[0][[1, 2, 0]]
    if extra_vertex:
        pos = np.vstack([pos, [[0.0, 0.0, 5.0]]])
    tex = None if uv is None else np.array([[uv * (p[0] + 1.0) / 2.0, (p[1] + 1.0) / 2.0] for p in pos], dtype=np.float64)
    nrm = np.tile([0.0, 0.0, 1.0], (len(pos), 1)) if normals else None
    return MeshData(pos, tris, nrm, "sheet", tex)


def build(**kw):
    # (texture coordinates reach the host scene only with a textured material)
    tex = Texture(np.arange(48, dtype=np.uint8).reshape(4, 4, 3)) if kw.get("uv") is not None else None
    red = Material(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0, texture=tex)
    kids = [Node.geo(Mesh(sheet(**kw)), red).translated((0.0, 0.5, 0.0)), Node.geo(Sphere(), red).translated((3.0, 0.0, 0.0))]
    return host_glue.host_scene(Scene(root=Node.group(kids), lights=[Light(position=(0.0, 8.0, 10.0), color=(0.9, 0.9, 0.9))], ambient=(0.1, 0.1, 0.1)))


def test_a_bent_mesh_has_the_same_topology_but_not_the_same_structure():
    a, b = build(), build(phase=0.8)
    same = a.same_topology(b)
    assert same and same.reason == ""
    assert a.same_topology(build())
    moved = a.same_structure(b)
    assert not moved and "another mesh" in moved.reason


def test_bent_texture_coordinates_and_normals_present_on_both_sides_keep_the_topology():
    assert build(uv=1.0, normals=True).same_topology(build(uv=1.0, normals=True, phase=0.4))


@pytest.mark.parametrize("what,change", [("one vertex more", dict(extra_vertex=True)), ("other triangles", dict(flip=True)), ("other texture coordinates", dict(uv=0.5)),
                                         ("normals appearing", dict(normals=True))])
def test_a_remeshed_scene_has_not(what, change):
    base = dict(uv=1.0) if "uv" in change else {}
    got = build(**base).same_topology(build(**{**base, "phase": 0.8, **change}))
    assert not got and "another mesh" in got.reason, what
