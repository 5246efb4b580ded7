"""pt_scene_update / Renderer.update: what can be checked without a GPU - the exports, the struct's layout, the bindings, the structure check of
Scene.same_structure (a scene may be moved, not rebuilt) and the argument check that needs no device."""
import ctypes as C
import math
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import Cube, Light, Material, MeshData, Mesh, Node, Scene, Sphere  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_libraries_export_the_update_entry_points():
    from portrayer_amd import _hip, host
    for name in ("pt_scene_update", "pt_node_scene_update"):
        assert hasattr(_hip.lib(), name), name
        assert name in _hip.EXPORTS and name in _hip.header_functions()
    for name in ("ph_renderer_update", "ph_scene_same_structure"):
        assert hasattr(host.lib(), name), name
        assert name in host.EXPORTS
    assert _hip.lib().pt_abi_version() == 8


def test_the_ctypes_struct_has_the_headers_fields_in_order():
    from portrayer_amd import _hip
    header = open(os.path.join(ROOT, "include", "portrayer_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} pt_scene_motion;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in decl.split(" ", 1 if decl.startswith("uint32_t") else 2)[-1].split(",")]
    assert names == [f[0] for f in _hip.PtSceneMotion._fields_]
    # 3 counts, each followed by pointers: 4 + pad, 3 x 8, 4 + pad, 3 x 8, 4 + pad, 2 x 8
    assert C.sizeof(_hip.PtSceneMotion) == 8 + 24 + 8 + 24 + 8 + 16
    assert _hip.PtSceneMotion.trans.offset == 8 and _hip.PtSceneMotion.n_graph_nodes.offset == 32 and _hip.PtSceneMotion.ambient.offset == 80


def test_the_python_bindings_exist():
    from portrayer_amd import host
    assert callable(host.Renderer.update) and callable(host.Scene.same_structure)


def test_a_null_context_is_refused_without_a_device():
    from portrayer_amd import _hip
    mo = _hip.PtSceneMotion()
    assert _hip.lib().pt_scene_update(None, C.byref(mo), None) == -1  # PT_ERR_ARGUMENT
    assert _hip.lib().pt_node_scene_update(None, C.byref(mo), None) == -1
    assert _hip.lib().pt_test_scene_bytes(None) == 0


RED = dict(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
BLUE = dict(diffuse=(0.2, 0.3, 0.8), specular=(0.3, 0.3, 0.3), shininess=25.0)


def tetrahedron(h=1.0):
    import numpy as np
    return MeshData(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, h]], dtype=np.float64), np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3], [0, 2, 3]], dtype=np.uint32))


def build(angle=0.0, shift=0.0, light=(0.0, 8.0, 10.0), extra=False, swap=False, mesh_h=1.0, blue_cube=False, more_light=False, regroup=False):
    red, blue = Material(**RED), Material(**BLUE)
    a = Node.geo(Cube() if swap else Sphere(), red).translated((-2.0 + shift, 1.0, 0.0))
    b = Node.geo(Sphere() if swap else Cube(), blue if blue_cube else red).scaled((1.0, 2.0 + shift, 1.0))
    m = Node.geo(Mesh(tetrahedron(mesh_h)), blue).translated((2.0, 0.0, shift))
    inner = [b] if regroup else [b, m]
    kids = [a, Node.group(inner).rotated_y(angle).translated((0.0, 0.0, -1.0))]
    if regroup:
        kids.append(Node.group([m]))
    if extra:
        kids.append(Node.geo(Sphere(), red).translated((5.0, 0.0, 0.0)))
    lights = [Light(position=light, color=(0.9, 0.9, 0.9))] + ([Light(position=(1.0, 2.0, 3.0), color=(0.1, 0.1, 0.1))] if more_light else [])
    return host_glue.host_scene(Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)))


def test_a_moved_scene_has_the_same_structure():
    same = build().same_structure(build(angle=math.pi / 3, shift=0.75, light=(3.0, 1.0, -2.0)))
    assert same and same.reason == ""


@pytest.mark.parametrize("what,change", [("one node more", dict(extra=True)), ("two nodes swapped in kind", dict(swap=True)), ("another mesh", dict(mesh_h=2.0)),
                                         ("another material", dict(blue_cube=True)), ("one light more", dict(more_light=True)),
                                         ("a child moved to another group", dict(regroup=True))])
def test_a_rebuilt_scene_has_not(what, change):
    got = build().same_structure(build(**change))
    assert not got and got.reason, what
