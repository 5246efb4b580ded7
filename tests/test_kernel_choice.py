"""Which render kernel a scene gets (pt_choose_kernel, csrc/pt_api.hip) against a table recorded from the code BEFORE the choice was one function
(tests/golden/kernel_choice/): every row is a small synthetic scene, whether it is textured and a set of environment switches, with the
(kernel_mode, kernel_variant) pt_stats reported for an 8 x 8 render of it then.

The CPU part asks pt_test_kernel_choice - no context, no device - for every row's choice from the row's traits. The GPU part builds, uploads and renders one
row per distinct (mode, variant), which pins the half the CPU part cannot see: how a scene becomes its traits."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from scene_dsl import GOLDEN, Camera, Cube, KDMesh, Light, Material, Mesh, MeshData, Node, Scene, Sphere, Texture

TABLE = os.path.join(GOLDEN, "kernel_choice", "table.json")

GEOMETRIES = ["spheres255", "spheres256", "mesh12", "mesh65534", "mesh65536", "kdmesh", "kdmesh+mesh65536"]
MATERIALS = ["matte", "mirror", "glossy", "glass", "glass+area"]
SWITCHES = ["", "PORTRAYER_WAVES=3", "PORTRAYER_WAVES=4", "PORTRAYER_WAVES=5", "PORTRAYER_KD_WAVES=3", "PORTRAYER_KD_WAVES=4", "PORTRAYER_KD_WAVES=5",
            "PORTRAYER_CHAIN=0", "PORTRAYER_CHAIN_WAVES=3", "PORTRAYER_CHAIN_WAVES=4", "PORTRAYER_PARK=0", "PORTRAYER_FORK=1", "PORTRAYER_PARK=0 PORTRAYER_FORK=1"]
SWITCH_NAMES = ("PORTRAYER_WAVES", "PORTRAYER_KD_WAVES", "PORTRAYER_CHAIN", "PORTRAYER_CHAIN_WAVES", "PORTRAYER_PARK", "PORTRAYER_FORK", "PORTRAYER_LDS_BUDGET_KB",
                "PORTRAYER_NO_TEX")
TRAITS = ("traverse", "n_nodes", "n_lights", "has_meshes", "has_kdmesh", "instanced_tris", "reflective", "reflective_opaque", "glossy", "area_light")


class PtSceneTraits(C.Structure):  # include/portrayer_hip.h: pt_scene_traits
    _fields_ = [("traverse", C.c_int32), ("n_nodes", C.c_uint32), ("n_lights", C.c_uint32), ("has_meshes", C.c_int32), ("has_kdmesh", C.c_int32),
                ("reflective", C.c_int32), ("reflective_opaque", C.c_int32), ("glossy", C.c_int32), ("area_light", C.c_int32), ("pad", C.c_int32),
                ("instanced_tris", C.c_uint64)]


def lights_of(geometry, material):
    """The light counts recorded for a scene: 32 and 33 only where the count can change the choice - it decides whether refracted subtrees may fork (32 lights or
    fewer), which needs glass without an area light; every other scene was recorded with one light (the trim the issue allows)."""
    return (1, 32, 33) if material == "glass" else (1,)


_MESHES = {}


def _grid_mesh(n_tris):
    """n_tris triangles of a grid of quads in the unit square of the xy-plane, with texture coordinates."""
    if n_tris not in _MESHES:
        side = int(np.ceil(np.sqrt(n_tris / 2.0)))
        u = np.arange(side + 1, dtype=np.float64) / side
        x, y = np.meshgrid(u, u, indexing="xy")
        pos = np.stack([x.ravel() - 0.5, y.ravel() - 0.5, np.zeros(x.size)], axis=1)
        i, j = np.meshgrid(np.arange(side), np.arange(side), indexing="xy")
        a = (j * (side + 1) + i).ravel()
        quads = np.stack([a, a + 1, a + side + 2, a, a + side + 2, a + side + 1], axis=1).reshape(-1, 3)
        _MESHES[n_tris] = MeshData(pos, quads[:n_tris].astype(np.uint32), None, "grid%d" % n_tris, pos[:, :2] + 0.5)
    return _MESHES[n_tris]


def build_scene(geometry, material, textured, n_lights):
    """-> (DSL scene, camera, traits without the traversal)"""
    mat = Material(diffuse=(0.7, 0.5, 0.3), specular=(0.2, 0.2, 0.2), shininess=10.0)
    if material == "mirror":
        mat.reflectivity = 0.8
    elif material == "glossy":
        mat.reflectivity = 0.8; mat.glossy_side_length = 0.2
    elif material in ("glass", "glass+area"):
        mat.reflectivity = 0.9; mat.refraction_index = 1.5
    if textured:
        mat.texture = Texture((np.arange(4 * 4 * 3, dtype=np.uint32) * 5 % 256).astype(np.uint8).reshape(4, 4, 3))
    kids, instanced, has_meshes, has_kdmesh = [], 0, False, False
    if geometry.startswith("spheres"):
        n = int(geometry[len("spheres"):])
        for k in range(n):
            kids.append(Node.geo(Sphere() if k % 2 else Cube(), mat).scaled(0.1).translated(((k % 16) * 0.3 - 2.4, (k // 16) * 0.3 - 2.4, 0.0)))
    for part in geometry.split("+"):
        if part == "kdmesh":
            kids.append(Node.geo(KDMesh(_grid_mesh(12)), mat).translated((-0.6, 0.0, 0.0)))
            instanced += 12; has_meshes = has_kdmesh = True
        elif part.startswith("mesh"):
            n = int(part[len("mesh"):])
            kids.append(Node.geo(Mesh(_grid_mesh(n)), mat).translated((0.6, 0.0, 0.0)))
            instanced += n; has_meshes = True
    lights = [Light(position=(3.0 * np.cos(k), 3.0 * np.sin(k), 5.0), color=(0.5, 0.5, 0.5)) for k in range(n_lights)]
    if material == "glass+area":
        lights[0].area_a = (0.5, 0.0, 0.0); lights[0].area_b = (0.0, 0.5, 0.0)
    reflective = material != "matte"
    traits = dict(n_nodes=len(kids), n_lights=n_lights, has_meshes=int(has_meshes), has_kdmesh=int(has_kdmesh), instanced_tris=instanced, reflective=int(reflective),
                  reflective_opaque=int(material not in ("glass", "glass+area")), glossy=int(material == "glossy"), area_light=int(material == "glass+area"))
    return Scene(Node.group(kids), lights, (0.1, 0.1, 0.1)), Camera((0.0, 0.0, 8.0), (0.0, 0.0, 0.0)), traits


def set_switches(monkeypatch, switch):
    for k in SWITCH_NAMES:
        monkeypatch.delenv(k, raising=False)
    for kv in switch.split():
        k, v = kv.split("=")
        monkeypatch.setenv(k, v)


def load_table():
    """-> rows (geometry, material, textured, n_lights, traits dict with the traversal, switch, mode, variant)"""
    with open(TABLE) as fh:
        t = json.load(fh)
    assert t["switches"] == SWITCHES and tuple(t["traits"]) == TRAITS
    rows = []
    for sc in t["scenes"]:
        traits = dict(zip(TRAITS, sc["traits"]))
        for switch, variant in zip(SWITCHES, sc["variants"]):
            rows.append((sc["geometry"], sc["material"], bool(sc["textured"]), traits["n_lights"], traits, switch, sc["mode"], variant))
    return rows


def test_the_table_covers_the_axes():
    rows = load_table()
    seen = {(r[0], r[1], r[2], r[3], r[4]["traverse"]) for r in rows}
    for tr in (1, 2, 3):  # PT_TRAVERSE_FLAT, _KD, _HIER
        for g in GEOMETRIES:
            for m in MATERIALS:
                for tex in (False, True):
                    for nl in lights_of(g, m):
                        assert (g, m, tex, nl, tr) in seen, (g, m, tex, nl, tr)


def test_every_row_gets_the_recorded_kernel(monkeypatch):
    from portrayer_amd import _hip as H
    fn = H.lib().pt_test_kernel_choice
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(PtSceneTraits), C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    rows = load_table()
    families, waves = set(), set()
    current = None
    for (g, m, tex, nl, traits, switch, mode, variant) in rows:
        if switch != current:
            set_switches(monkeypatch, switch)
            current = switch
        t = PtSceneTraits(**traits)
        got_mode, got_variant = C.c_uint32(), C.c_uint32()
        assert fn(C.byref(t), -1, int(tex), C.byref(got_mode), C.byref(got_variant)) == 0
        assert (got_mode.value, got_variant.value) == (mode, variant), (g, m, tex, nl, traits, switch)
        w = variant & H.KERNEL_WAVES_MASK
        waves.add(w)
        if variant & H.KERNEL_CHAIN:
            families.add("chain")
        elif variant & H.KERNEL_FORK:
            families.add("interp_fork")
        elif variant & H.KERNEL_PARK:
            families.add("interp_park")
        elif variant & H.KERNEL_INTERPRETER:
            families.add("interp")
        else:
            families.add("line%d" % min(w, 5))
    assert families == {"interp", "interp_park", "interp_fork", "chain", "line3", "line4", "line5"}  # every PT_RUN_* (LINE5: the densest instantiation, 5 or 6 waves)
    assert waves == {3, 4, 5, 6}


def _distinct_rows():
    if not os.path.exists(TABLE):
        return []
    first = {}
    for r in load_table():
        first.setdefault((r[6], r[7]), r)
    return [first[k] for k in sorted(first)]


@pytest.mark.gpu
@pytest.mark.parametrize("row", _distinct_rows(), ids=lambda r: "mode%d-variant%d" % (r[6], r[7]))
def test_a_scene_of_the_row_runs_the_recorded_kernel(monkeypatch, row):
    import host_glue
    from portrayer_amd import host
    g, m, tex, nl, traits, switch, mode, variant = row
    set_switches(monkeypatch, switch)
    scene, cam, _ = build_scene(g, m, tex, nl)
    r = host.Renderer(host_glue.host_scene(scene), traits["traverse"], kd_depth=4)
    try:
        st = r.render(host_glue.cam10(cam), 8, 8, np.zeros((8, 3)), samples=1, seed=1)[2]
    finally:
        r.close()
    assert (st["kernel_mode"], st["kernel_variant"]) == (mode, variant), (g, m, tex, nl, switch)
