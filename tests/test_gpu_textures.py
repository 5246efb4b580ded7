"""Image textures and normal maps (src/texture.rs, consumed at material.rs:109-144) on
the GPU against the oracle and the reference's golden render of examples/normal-mapping.rs."""
import os

import numpy as np
import pytest
from PIL import Image

import host_glue
from example_scenes import load_mesh, normal_mapping
from scene_dsl import (GOLDEN, Camera, Cube, Cylinder, Light, Material, Mesh, Node, Plane, Scene, Sphere, Texture, Triangle, default_background,
                       to_radians)

pytestmark = pytest.mark.gpu


from ulp import assert_ulp, ulp_diff  # noqa: E402


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def texel_edge_proof(ref):
    """Sphere texture coordinates go through libm's atan2 / acos (sphere.rs:59-96); the device's routines are within 2 / 1 ulp of glibc's, not bit-equal,
    and glibc's own are not correctly rounded, so nothing short of glibc's instruction sequence reproduces them. A texel can only differ where
    u (w - 1) or v (h - 1) lies within a few ulps of an integer. The oracle counts the texel fetches whose coordinates came from a sphere hit and those of
    them within 4096 ulps of a texel edge (po_stats, round 5): none near an edge = the device fetched the same texels, so the comparison below is EXACT -
    the "<= 2 pixels may differ" of rounds 1 - 4 is gone."""
    assert ref.stats["tex_sphere_near_edge"] == 0, "a sphere's texture coordinate lies within 4096 ulps of a texel edge: pick another seed / size for this test"
    return ref.stats["tex_sphere_lookups"]


def block_means(a, k=8):
    h, w, _ = a.shape
    h2, w2 = h // k * k, w // k * k
    return a[:h2, :w2].astype(float).reshape(h2 // k, k, w2 // k, k, 3).mean(axis=(1, 3))


@pytest.mark.parametrize("mode", ["flat", "kd"])
def test_normal_mapping_example_matches_oracle(oracle, host, H, mode):
    scene, cam, _ = normal_mapping()
    w, h = 455, 256
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_KD if mode == "kd" else H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), stats=True)
    ref = oracle.render(scene, cam, w, h, mode=oracle.MODE_KD if mode == "kd" else oracle.MODE_FLAT)
    assert st["hits"] == ref.stats["hits"] and st["shadow"] == ref.stats["shadow"]
    assert texel_edge_proof(ref) > 0  # (the scene's normal-mapped sphere)
    assert np.array_equal(rgb, ref.rgb), f"{(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
    assert_ulp(linear, ref.linear, 0)


def test_gpu_normal_mapping_vs_reference_golden(host, H):
    """render/04a_normal-mapping.png was rendered with many jittered samples from JPEG textures decoded by
    another decoder: compare 8x8 block means of a centre-sample GPU render (measured on the oracle: mean
    1.1 levels, 3 % of blocks above 6, all on the top edge of the left wall)."""
    scene, cam, (w, h) = normal_mapping()
    g = np.array(Image.open(os.path.join(GOLDEN, "render", "04a_normal-mapping.png")).convert("RGB"))
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    rgb, _, _ = r.render(host_glue.cam10(cam), w, h, default_background(w, h), want_linear=False)
    d = np.abs(block_means(rgb) - block_means(g)).max(axis=2)
    assert d.mean() < 1.5 and (d > 6).mean() < 0.05


def textured_scene(seed):
    rng = np.random.default_rng(seed)
    tex_a = Texture(rng.integers(0, 256, (37, 53, 3), dtype=np.uint8))
    tex_b = Texture(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8))
    nm = rng.integers(0, 256, (48, 32, 3), dtype=np.uint8); nm[..., 2] = np.maximum(nm[..., 2], 140)  # normals pointing out of the surface
    nmap = Texture(nm)
    m_cube = Material(diffuse=(0.5, 0.5, 0.5), specular=(0.4, 0.4, 0.4), shininess=30.0, texture=tex_a, normals=nmap)
    m_sphere = Material(diffuse=(0.2, 0.8, 0.2), specular=(0.5, 0.5, 0.5), shininess=10.0, texture=tex_b, reflectivity=0.4,
                        uv_trans=(2.0, 0.0, 0.25, 0.0, 3.0, -0.5, 0.0, 0.0, 1.0))
    m_plane = Material(diffuse=(0.9, 0.9, 0.9), texture=tex_a, uv_trans=(4.0, 0.0, 0.0, 0.0, 4.0, 0.0, 0.0, 0.0, 1.0))
    m_tri = Material(diffuse=(1, 1, 1), specular=(0.3, 0.3, 0.3), shininess=5.0, texture=tex_b, normals=nmap)
    m_mesh = Material(diffuse=(1, 1, 1), specular=(0.2, 0.2, 0.2), shininess=50.0, texture=tex_b)
    m_plain = Material(diffuse=(0.8, 0.3, 0.3), specular=(0.3, 0.3, 0.3), shininess=25.0)
    monkey = load_mesh("monkey.obj")  # has vt records
    assert monkey.tex_coords is not None
    tri = Triangle((-1.5, 0.0, 0.0), (1.5, 0.0, 0.0), (0.0, 2.0, 0.5), normals=rng.uniform(-1, 1, (3, 3)) + np.array([0, 0, 2.0]),
                   tex_coords=[(0.0, 0.0), (1.0, 0.1), (0.4, 1.3)])
    root = Node.group([
        Node.geo(Plane(), m_plane).scaled(14.0).translated((0.0, -1.0, 0.0)),
        Node.geo(Cube(), m_cube).scaled((1.5, 2.0, 1.0)).rotated_y(0.5).translated((-3.0, 0.0, 0.0)),
        Node.geo(Sphere(), m_sphere).scaled(1.2).rotated_xzy((0.3, 0.9, -0.4)).translated((0.0, 0.3, 0.5)),
        Node.geo(tri, m_tri).translated((3.0, -0.8, 0.0)),
        Node.geo(Mesh(monkey, smooth=bool(seed % 2)), m_mesh).rotated_y(to_radians(150.0 + 20 * seed)).translated((0.5, 2.3, -1.0)),
        Node.geo(Cylinder(), m_plain).translated((-1.2, -0.5, 2.0)),
    ])
    lights = [Light(position=(4.0, 7.0, 8.0), color=(0.8, 0.8, 0.8)), Light(position=(-6.0, 5.0, 3.0), color=(0.3, 0.3, 0.5))]
    return Scene(root=root, lights=lights, ambient=(0.25, 0.25, 0.25)), Camera(eye=(0.5, 3.0, 10.0), center=(0.0, 0.5, 0.0), fovy_degrees=38.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["flat", "kd"])
def test_random_textured_scene_matches_oracle(oracle, host, H, seed, mode):
    scene, cam = textured_scene(seed)
    w, h = 160, 110
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_KD if mode == "kd" else H.TRAVERSE_FLAT, kd_depth=5)
    kw = dict(samples=2, seed=seed, sample_mode=H.SAMPLE_RNG) if seed else {}
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), stats=True, **kw)
    okw = dict(samples=2, seed=seed, jitter=oracle.JITTER_RNG) if seed else {}
    ref = oracle.render(scene, cam, w, h, mode=oracle.MODE_KD if mode == "kd" else oracle.MODE_FLAT, kd_depth=5, **okw)
    for k in ("primary", "shadow", "reflect", "hits"):
        assert st[k] == ref.stats[k], k
    assert ref.stats["kd_plane_miss"] == 0
    texel_edge_proof(ref)
    bad = (rgb != ref.rgb).any(axis=2)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ, first at {np.argwhere(bad)[:3]}"
    assert_ulp(linear, ref.linear, 0)


@pytest.mark.parametrize("seed", [0, 1])
def test_four_wave_chain_kernel_of_hierarchical_textured_mesh_scenes_matches_oracle(oracle, host, H, monkeypatch, seed):
    """PORTRAYER_CHAIN_WAVES=4 on a textured scene with Mesh instances and an opaque mirror in the hierarchical semantics: the chain
    kernels pt_render_simple_kernel<8, *, true, 4, true>, whose blocks .LBB5_51 (counting) and .LBB13_796 (plain) the build repairs
    (tools/check_exec_prologue.py). Both exact against the oracle."""
    for k in ("PORTRAYER_PARK", "PORTRAYER_CHAIN", "PORTRAYER_NO_TEX"):  # this test picks the kernels itself (tests/test_gpu_switch_matrix.py)
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PORTRAYER_CHAIN_WAVES", "4")
    scene, cam = textured_scene(seed)
    w, h = 160, 110
    bg = default_background(w, h)
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_HIER)
    kw = dict(samples=2, seed=seed, sample_mode=H.SAMPLE_RNG)
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, bg, stats=False, **kw)
    counted, counted_linear, stc = r.render(host_glue.cam10(cam), w, h, bg, stats=True, **kw)
    r.close()
    want = H.KERNEL_CHAIN | H.KERNEL_TEXTURED | 4
    assert st["kernel_mode"] == stc["kernel_mode"] == 8
    assert st["kernel_variant"] & (want | H.KERNEL_COUNTING | H.KERNEL_WAVES_MASK | H.KERNEL_INTERPRETER) == want
    assert stc["kernel_variant"] & (want | H.KERNEL_COUNTING | H.KERNEL_WAVES_MASK | H.KERNEL_INTERPRETER) == want | H.KERNEL_COUNTING
    ref = oracle.render(scene, cam, w, h, samples=2, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_HIER)
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert stc[k] == ref.stats[k], k
    assert ref.stats["reflect"] > 0
    texel_edge_proof(ref)
    for img, lin in [(rgb, linear), (counted, counted_linear)]:
        bad = (img != ref.rgb).any(axis=2)
        assert bad.sum() == 0, f"{bad.sum()} pixels differ, first at {np.argwhere(bad)[:3]}"
        assert_ulp(lin, ref.linear, 0)


def test_texture_on_primitive_without_uv_is_rejected(host, H):
    """material.rs:133 / :141: 'Texture mapping is not supported for this primitive!' (a panic in the reference)."""
    tex = Texture(np.zeros((4, 4, 3), dtype=np.uint8))
    scene = Scene(root=Node.group([Node.geo(Cylinder(), Material(diffuse=(1, 1, 1), texture=tex))]), lights=[], ambient=(1, 1, 1))
    with pytest.raises(host.PortrayerHostError):
        host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)


def test_cpp_fish_example_matches_oracle(oracle, host, H):
    """examples/fish.cpp end to end: the C++ host's own PNG decoder (RGBA -> RGB) and OBJ reader (`vt` records,
    v flipped like triangle.rs:134-137) feed the device; the oracle gets the same scene from the test DSL
    (PIL-decoded texture, Python OBJ reader). Textured, smooth-shaded mesh: uv interpolation + nearest texel."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import ASSETS, default_background
    sc = host.Scene.example("fish", assets=ASSETS)
    scene, cam, size = TEXTURED_EXAMPLES["fish"]()
    assert sc.size == size
    w, h = 455, 256
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(sc.camera, w, h, default_background(w, h), samples=2, seed=5, sample_mode=H.SAMPLE_RNG, stats=True)
    ref = oracle.render(scene, cam, w, h, samples=2, seed=5, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert st["hits"] == ref.stats["hits"] > 1000
    assert np.array_equal(rgb, ref.rgb)
    r.close()


def test_cpp_transmission_refraction_example_matches_oracle(oracle, host, H):
    """examples/transmission-refraction.cpp end to end (C++ JPEG / PNG / OBJ readers, KDMesh trees built by the C++ host)."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import ASSETS, default_background
    sc = host.Scene.example("transmission-refraction", assets=ASSETS)
    scene, cam, size = TEXTURED_EXAMPLES["transmission-refraction"]()
    assert sc.size == size
    w, h = 364, 204
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(sc.camera, w, h, default_background(w, h), samples=2, seed=4, sample_mode=H.SAMPLE_RNG, stats=True)
    ref = oracle.render(scene, cam, w, h, samples=2, seed=4, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    assert np.array_equal(rgb, ref.rgb)
    r.close()


def test_cpp_water_glass_example_matches_oracle(oracle, host, H):
    """examples/water-glass.cpp end to end: glossy reflection draws + refraction + normal-mapped textures (JPEG, one of
    them 1025 x 1025 with 4:2:0 chroma)."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import ASSETS, default_background
    sc = host.Scene.example("water-glass", assets=ASSETS)
    scene, cam, size = TEXTURED_EXAMPLES["water-glass"]()
    assert sc.size == size
    w, h = 455, 256
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(sc.camera, w, h, default_background(w, h), samples=3, seed=2, sample_mode=H.SAMPLE_RNG, stats=True)
    ref = oracle.render(scene, cam, w, h, samples=3, seed=2, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    assert np.array_equal(rgb, ref.rgb)
    r.close()


def test_cpp_normal_mapping_example_matches_oracle(oracle, host, H):
    """examples/normal-mapping.cpp end to end: six JPEG files (baseline and progressive) decoded by the C++ host,
    texture + normal maps on Plane, Cube and Sphere; the oracle gets the scene from the test DSL with
    Pillow-decoded texels - the two decoders agree bit for bit, so the images must be identical."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import ASSETS, default_background
    sc = host.Scene.example("normal-mapping", assets=ASSETS)
    scene, cam, size = TEXTURED_EXAMPLES["normal-mapping"]()
    assert sc.size == size
    w, h = 455, 256
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(sc.camera, w, h, default_background(w, h), samples=2, seed=9, sample_mode=H.SAMPLE_RNG, stats=True)
    ref = oracle.render(scene, cam, w, h, samples=2, seed=9, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert st["hits"] == ref.stats["hits"] > 1000
    assert np.array_equal(rgb, ref.rgb)
    r.close()


@pytest.mark.parametrize("mode", ["flat", "kd"])
def test_transmission_refraction_matches_oracle(oracle, host, H, mode):
    """The reference's most demanding scene script in one piece: glass and water (refraction to depth 10), textured
    KDMesh fish, texture + normal maps on cubes, coincident faces (quirk Q13: ties decided by the last bit, so both
    sides must round identically)."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import default_background
    scene, cam, _ = TEXTURED_EXAMPLES["transmission-refraction"]()
    w, h = 364, 204
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_KD if mode == "kd" else H.TRAVERSE_FLAT)
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), samples=2, seed=4, sample_mode=H.SAMPLE_RNG, stats=True)
    ref = oracle.render(scene, cam, w, h, samples=2, seed=4, jitter=oracle.JITTER_RNG, mode=oracle.MODE_KD if mode == "kd" else oracle.MODE_FLAT)
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    assert np.array_equal(rgb, ref.rgb)
    r.close()


@pytest.mark.parametrize("scene_name,mode", [("textured-1", "flat"), ("textured-1", "kd"), ("transmission-refraction", "flat"),
                                             ("transmission-refraction", "hier"), ("water-glass", "hier")])
def test_recursion_frames_all_in_hbm(oracle, host, H, monkeypatch, scene_name, mode):
    """Scenes with reflective materials run the PARK = 1 instantiations (a lane's youngest parked recursion frame stays in
    LDS, older ones go to HBM). PORTRAYER_PARK=0 forces the instantiations that keep every parked frame in HBM, which
    such scenes otherwise never run; results must not depend on where a frame waits."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import default_background
    monkeypatch.setenv("PORTRAYER_PARK", "0")
    scene, cam = textured_scene(1) if scene_name == "textured-1" else TEXTURED_EXAMPLES[scene_name]()[:2]
    tr, om = {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]
    w, h = 200, 112
    r = host.Renderer(host_glue.host_scene(scene), tr, kd_depth=5)
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, default_background(w, h), samples=2, seed=8, sample_mode=H.SAMPLE_RNG, stats=True)
    plain, _, _ = r.render(host_glue.cam10(cam), w, h, default_background(w, h), samples=2, seed=8, sample_mode=H.SAMPLE_RNG)  # the non-counting instantiation
    ref = oracle.render(scene, cam, w, h, samples=2, seed=8, jitter=oracle.JITTER_RNG, mode=om, kd_depth=5)
    r.close()
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    bad = (rgb != ref.rgb).any(axis=2)
    texel_edge_proof(ref)
    assert bad.sum() == 0
    assert np.array_equal(plain, rgb)


@pytest.mark.parametrize("scene_name,mode", [("transmission-refraction", "flat"), ("transmission-refraction", "hier"), ("transmission-refraction", "kd")])
def test_fork_join_of_refracted_subtrees_matches_oracle(oracle, host, H, monkeypatch, scene_name, mode):
    """PORTRAYER_FORK=1: lanes whose samples are finished take the refracted subtrees busy lanes offer (LDS queue, ballot ranks,
    mailboxes in HBM; pt_shade.h). Which lane walks a subtree must not change a bit: image, f64 means and ray counts == the oracle's,
    and == the render without forking. 64 samples per pixel: a wavefront is one pixel, offers and idle lanes meet inside it."""
    from example_scenes import TEXTURED_EXAMPLES
    from scene_dsl import default_background
    for k in ("PORTRAYER_FORK", "PORTRAYER_PARK"):  # this test picks the kernels itself
        monkeypatch.delenv(k, raising=False)
    scene, cam = TEXTURED_EXAMPLES[scene_name]()[:2]
    tr, om = {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]
    w, h, samples = 96, 54, 64
    bg = default_background(w, h)
    r = host.Renderer(host_glue.host_scene(scene), tr, kd_depth=5)
    plain, plain_linear, st0 = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG, stats=True)
    assert not st0["kernel_variant"] & H.KERNEL_FORK
    monkeypatch.setenv("PORTRAYER_FORK", "1")
    rgb, linear, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG, stats=True)
    fast, fast_linear, st2 = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG)  # the non-counting instantiation
    r.close()
    assert st["kernel_variant"] & H.KERNEL_FORK and st2["kernel_variant"] & H.KERNEL_FORK
    assert np.array_equal(rgb, plain) and np.array_equal(linear, plain_linear), "forking changed the picture"
    assert np.array_equal(fast, rgb) and np.array_equal(fast_linear, linear)
    for k in ("primary", "shadow", "reflect", "refract", "hits", "depth11_skipped"):
        assert st[k] == st0[k], k
    ref = oracle.render(scene, cam, w, h, samples=samples, seed=3, jitter=oracle.JITTER_RNG, mode=om, kd_depth=5)
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    assert np.array_equal(rgb, ref.rgb)
