"""pt_scene_upload = pt_upload_prepare, then pt_upload_commit (csrc/pt_scene.hip): every refusal the host can decide comes before the first HIP call, with the
words it has always had, and a refused upload leaves the context without a scene and its device buffers as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "portrayer_amd", "csrc", "pt_scene.hip")

# step of pt_upload_prepare (in the order it runs them) -> the refusals it holds, in the order it checks them
STEPS = [
    ("pt_upload_prepare", ["traverse must be PT_TRAVERSE_FLAT, PT_TRAVERSE_KD or PT_TRAVERSE_HIER", "PT_TRAVERSE_HIER needs the scene graph (graph_*, node_chain*, node_dfs_rank)",
                           "PT_TRAVERSE_KD needs the host-built k-d tree", "null node array"]),
    ("pt_upload_check_nodes", ["unknown primitive type", "material index out of range", "mesh index out of range",
                               "smooth shading needs a vertex normal per vertex (mesh.rs:135-138)", "triangle index out of range", "triangle normals missing"]),
    ("pt_upload_pack_triangles", []),
    ("pt_upload_pack_mesh", ["meshes must have at least one vertex (mesh.rs:71)", "mesh index out of range", "mesh_bounds_invtrans missing"]),
    ("pt_upload_pack_kdmeshes", ["incomplete KDMesh tree arrays", "KDMesh tree child out of range", "KDMesh leaf range out of bounds"]),
    ("pt_upload_pack_kdmesh", ["KDMesh root out of range", "KDMesh trees must not share nodes", "KDMesh leaf triangle out of range"]),
    ("pt_upload_pack_nodes", ["node_chain_off must start at 0", "every flattened node needs a non-empty path (it contains at least itself)",
                              "node_chain names a graph node out of range"]),
    ("pt_upload_pack_scene_tree", []),
    ("pt_pack_kd", ["incomplete k-d tree", "k-d child out of range", "k-d leaf range out of bounds", "k-d leaf item out of range", "k-d tree is not a tree",
                    "k-d tree deeper than 32 levels (the limit of the k-d walk: include/portrayer_hip.h, pt_kdtree)", "k-d tree of 2^26 nodes or more",
                    "k-d tree with 2^27 leaf references or more"]),
    ("pt_upload_check_tree_size", ["too many triangles for the 32-bit tree references (a node is addressed by a 32-bit byte offset: 2^26 nodes)"]),
    ("pt_upload_pack_shading", []),
    ("pt_upload_pack_textures", ["textured material without texture data", "empty texture", "texture index out of range",
                                 "Texture mapping is not supported for this primitive! (material.rs:133,141)"]),
]
TEXTURE_REFUSAL = "Texture mapping is not supported for this primitive! (material.rs:133,141)"


def function_body(text, name):
    """The static function `name` of the source, from its signature to its closing brace in column 0."""
    m = re.search(r"^static [\w:<>&\* ]+\b%s\(" % re.escape(name), text, flags=re.M)
    assert m, name
    return text[m.start():text.index("\n}\n", m.start())]


def test_the_host_side_refusals_keep_their_words_and_come_before_any_hip_call():
    src = open(SOURCE).read()
    prepare = function_body(src, "pt_upload_prepare")
    called = []
    for name, words in STEPS:
        body = function_body(src, name)
        assert "hip" not in body.replace("portrayer_hip.h", "") and "PT_HIP" not in body and "pt_reserve" not in body and "pt_upload(" not in body, name
        at = [body.index('"%s"' % w) for w in words]
        assert at == sorted(at), name
        if name not in ("pt_upload_prepare", "pt_upload_pack_mesh", "pt_upload_pack_kdmesh"):  # (the per-mesh steps are called by the steps in front of them)
            called.append(prepare.index(name + "("))
    assert called == sorted(called)
    assert prepare.index("c->have_scene = false;") < called[0]
    upload = src[src.index('extern "C" int pt_scene_upload('):]
    upload = upload[:upload.index("\n}\n")]
    assert upload.index("pt_upload_prepare(") < upload.index("pt_upload_commit(") and "hip" not in upload
    commit = function_body(src, "pt_upload_commit")
    assert commit.index("hipSetDevice") < commit.index("pt_upload_commit_trees(") and commit.rindex("c->have_scene = true;") > commit.index("pt_set_stack_cap(")


@pytest.mark.gpu
def test_a_textured_cylinder_is_refused_before_anything_is_written():
    import device_glue
    from portrayer_amd import _hip as H
    from scene_dsl import Cylinder, Light, Material, Node, Scene, Sphere
    lib = H.lib()
    plain, mapped = Material(diffuse=(0.5, 0.5, 0.5)), Material(diffuse=(0.2, 0.6, 0.2))
    scene = Scene(Node.group([Node.geo(Sphere(), plain).translated((-1.0, 0.0, 0.0)), Node.geo(Cylinder(), mapped).translated((1.0, 0.0, 0.0))]),
                  [Light(position=(0.0, 5.0, 5.0), color=(1.0, 1.0, 1.0))], (0.1, 0.1, 0.1))
    ds = device_glue.DeviceScene(scene)
    assert ds.struct.n_nodes == 2 and ds.keep["type"][1] == 6 and ds.keep["mat"][1] == 1  # the second node: a cylinder with the second material
    ctx = H.Context(0)
    try:
        ds.upload(ctx)
        info = (C.c_uint64 * 4)()
        assert lib.pt_test_scene_info(ctx.handle, C.byref(info)) == 0
        before = lib.pt_test_scene_bytes(ctx.handle)
        # the same scene with a texture on the cylinder's material
        tex = np.array([-1, 0], dtype=np.int32)
        size, offset, rgb = np.array([2, 2], dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.full(12, 128, dtype=np.uint8)
        s = ds.struct
        s.material_texture = tex.ctypes.data_as(H._ip)
        s.n_textures = 1
        s.texture_size, s.texture_offset, s.texture_rgb = size.ctypes.data_as(H._up), offset.ctypes.data_as(H._u64p), rgb.ctypes.data_as(H._u8p)
        assert lib.pt_scene_upload(ctx.handle, C.byref(s), H.TRAVERSE_FLAT, None) == H.ERR_SCENE
        assert lib.pt_last_error(ctx.handle).decode() == TEXTURE_REFUSAL
        assert lib.pt_test_scene_bytes(ctx.handle) == before  # nothing was allocated
        assert lib.pt_test_scene_info(ctx.handle, C.byref(info)) == H.ERR_NO_SCENE  # and the context has no scene
    finally:
        ctx.close()
