"""Textures, normal maps and uv_trans on the device (Renderer.radiance, Renderer.render, Renderer.guides) against the exact-arithmetic reference's
colours and texels in tests/golden/exact_textures/.

Reads the fixtures and tolerances.json only (tools/gen_exact_textures.py wrote them from tests/exact_shade.py; see tests/test_exact_textures.py for what
they hold). On every ray the exact reference can decide, in all three traversals, the colour lies within the scene's threshold per channel,
|d| / max(1, |c|), and equals po_color_rays' bits. render() of the camera batch runs the straight-line kernels in tex_prims, tex_nested and tex_tris, the
chain kernel in tex_mirror and the interpreter (pt_lane_maps) in tex_glass. The albedo of the guides pass is the exact texel's colour, bit for bit.
Every test traces at most 540 rays or renders 16 x 12 pixels."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_shading as G  # noqa: E402
import gen_exact_textures as T  # noqa: E402
import host_glue  # noqa: E402
from test_exact_shading import oracle_colors  # noqa: E402
from test_exact_textures import pow_as_the_kernels  # noqa: E402
from test_gpu_aov import bits  # noqa: E402
from test_gpu_exact_shading import check, same_bits, traversal  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = T.load_tolerances()
MODES = ("flat", "kd", "hier")
CASES = [(s, b) for s in T.SCENES for b in T.BATCH_NAMES]
KERNEL = {"tex_prims": "line", "tex_nested": "line", "tex_tris": "line", "tex_mirror": "chain", "tex_glass": "interpreter"}


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(scope="module")
def scenes(oracle):
    out = {}
    for s in T.SCENES:
        scene = T.build_scene(s)
        ps = oracle.pack(scene)
        bs = {b: T.load(s, b) for b in T.BATCH_NAMES}
        assert oracle.flatten(ps)["trans"].tobytes() == bs["camera"]["trans"].tobytes(), "%s is not the scene of the fixture" % s
        assert all(len(c["o"]) <= 540 for c in bs.values())
        out[s] = dict(scene=scene, host=host_glue.host_scene(scene), ps=ps, batches=bs)
    return out


@pytest.fixture(scope="module")
def oracle_bits(oracle, scenes):
    """po_color_rays' colours of a batch, computed once."""
    cache = {}

    def get(scene, name, mode):
        if (scene, name, mode) not in cache:
            c = scenes[scene]["batches"][name]
            cache[scene, name, mode] = oracle_colors(oracle, scenes[scene]["ps"], c["o"], c["d"], c["bg"], mode)
        return cache[scene, name, mode]
    return get


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene,name", CASES)
def test_radiance_is_the_exact_colour(host, H, scenes, oracle_bits, scene, name, mode, reorder):
    s, c = scenes[scene], scenes[scene]["batches"][name]
    r = host.Renderer(s["host"], traversal(H, mode), kd_depth=T.KD_DEPTH)
    got = r.radiance(c["o"], c["d"], background=c["bg"], seed=0, sample=0, stream_base=0, reorder=reorder)["rgb"]
    r.close()
    tag = "%s %s %s reorder=%d" % (scene, name, mode, reorder)
    check(tag, c, got, TOL[scene], mode, name)
    same_bits(got, oracle_bits(scene, name, mode), tag + " vs po_color_rays")   # so both orders give the same bits


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", T.BATCH_NAMES)
def test_glass_with_every_recursion_frame_in_hbm(host, H, scenes, oracle_bits, monkeypatch, name, mode, reorder):
    """PORTRAYER_PARK=0 (read at every call): no parked frame stays in LDS; a frame carries the hit's texture coordinates and basis with it."""
    c = scenes["tex_glass"]["batches"][name]
    r = host.Renderer(scenes["tex_glass"]["host"], traversal(H, mode), kd_depth=T.KD_DEPTH)
    monkeypatch.setenv("PORTRAYER_PARK", "0")
    in_hbm = r.radiance(c["o"], c["d"], background=c["bg"], reorder=reorder)["rgb"]
    monkeypatch.delenv("PORTRAYER_PARK")
    r.close()
    tag = "tex_glass %s %s reorder=%d, frames in HBM" % (name, mode, reorder)
    check(tag, c, in_hbm, TOL["tex_glass"], mode, name)
    same_bits(in_hbm, oracle_bits("tex_glass", name, mode), tag + " vs po_color_rays (as with the youngest frame in LDS)")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", T.SCENES)
def test_render_is_the_exact_colour_of_the_eye_rays(host, H, scenes, scene, mode):
    c = scenes[scene]["batches"]["camera"]
    w, h = (int(x) for x in c["size"])
    assert w * h == len(c["o"]) <= 16 * 12
    r = host.Renderer(scenes[scene]["host"], traversal(H, mode), kd_depth=T.KD_DEPTH)
    _, linear, st = r.render(c["cam"], w, h, c["bg"].reshape(h, w, 3), samples=1, seed=0, sample_mode=H.SAMPLE_CENTRE)
    r.close()
    check("%s render %s" % (scene, mode), c, linear.reshape(-1, 3), TOL[scene], mode, "camera")
    v = st["kernel_variant"]
    kernel = "chain" if v & H.KERNEL_CHAIN else ("interpreter" if v & H.KERNEL_INTERPRETER else "line")
    assert kernel == KERNEL[scene], "%s %s ran the %s kernel (variant %d)" % (scene, mode, kernel, v)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", T.SCENES)
def test_albedo_is_the_exact_texel(host, H, scenes, scene, mode):
    """Where the primary hit is textured and decidable the albedo is (byte / 255) ^ 2.2 of the fixture's exact texel bytes, bit for bit (whatever the
    material reflects); where it is not textured, the material's diffuse colour; +0 on a miss."""
    c = scenes[scene]["batches"]["camera"]
    w, h = (int(x) for x in c["size"])
    r = host.Renderer(scenes[scene]["host"], traversal(H, mode), kd_depth=T.KD_DEPTH)
    got = r.guides(c["cam"], w, h, want=("albedo", "node"))
    r.close()
    albedo, node = got["albedo"].reshape(-1, 3), got["node"].reshape(-1)
    ok = G.decidable(c, mode)
    rgb, textured = T.texel_bytes(c)
    which = ok & textured
    assert int(which.sum()) >= 48, "%s: only %d eye rays meet a textured surface" % (scene, int(which.sum()))
    exp = pow_as_the_kernels((rgb[which] / 255.0).ravel(), 2.2).reshape(-1, 3)
    wrong = np.flatnonzero(np.any(bits(albedo[which]) != bits(exp), axis=1))
    assert wrong.size == 0, "%s %s: %d texels differ, first at pixel %d: exact bytes %s give %s, the device has %s" % (
        scene, mode, wrong.size, int(np.flatnonzero(which)[wrong[0]]), rgb[which][wrong[0]].tolist(), exp[wrong[0]].tolist(), albedo[which][wrong[0]].tolist())
    assert np.array_equal(node[ok], c["node"][ok]), "%s %s: primary hits" % (scene, mode)
    miss = ok & ~c["hit"]
    assert not bits(albedo[miss]).any(), "misses must hold +0"
    plain = ok & c["hit"] & ~textured
    diffuse = np.array([m.diffuse for m in G.flat_materials(scenes[scene]["scene"])], dtype=np.float64)
    assert np.array_equal(bits(albedo[plain]), bits(diffuse[c["node"][plain]])), "%s %s: untextured hits" % (scene, mode)
