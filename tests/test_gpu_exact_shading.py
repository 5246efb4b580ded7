"""Shading on the device (Renderer.radiance, Renderer.render) against the exact-arithmetic reference's colours in tests/golden/exact_shading/.

Reads the fixtures and tolerances.json only (tools/gen_exact_shading.py wrote them from tests/exact_shade.py; see tests/test_exact_shading.py for what they
hold and how the thresholds were measured). On every ray the exact reference can decide, in all three traversals, the colour lies within the scene's
threshold per channel, |d| / max(1, |c|); in the k-d traversal the exact answer is the exact walk of the scene's k-d tree, in the hierarchical one the
exact walk of the hierarchy. Fragile and badly conditioned rays are traced, left out of the comparison and counted against the caps. Ray i draws from
stream (0, i, 0) and has its own background colour, a function of i. Every test traces at most 540 rays or renders at most 16 x 12 pixels: the order,
the slices and the frames in HBM are tests of their own, each held to po_color_rays' bits, which are computed once per scene, batch and traversal
(ray i behind i placeholder rays, tests/test_exact_shading.py: oracle_colors)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_shading as G  # noqa: E402
import host_glue  # noqa: E402
from test_exact_shading import oracle_colors  # noqa: E402
from test_gpu_aov import bits  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = G.load_tolerances()
MODES = ("flat", "kd", "hier")
CASES = [(s, b) for s in G.SCENES for b in G.batches_of(s)]
# what render() runs per scene: straight-line kernels without reflective materials, the chain kernel where every reflective material is opaque and not
# glossy (one secondary ray per hit), else the interpreter
KERNEL = {"lit15": "interpreter", "lit_nested": "interpreter", "hall": "interpreter", "hall_opaque": "chain", "lit_tris": "line", "many65": "line", "tangent": "line"}


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
    for s in G.SCENES:
        scene = G.build_scene(s)
        ps = oracle.pack(scene)
        bs = {b: G.load(s, b) for b in G.batches_of(s)}
        assert oracle.flatten(ps)["trans"].tobytes() == bs["camera"]["trans"].tobytes(), "%s is not the scene of the fixture" % s
        assert all(len(c["o"]) <= 540 for c in bs.values())
        out[s] = dict(host=host_glue.host_scene(scene), ps=ps, batches=bs)
    return out


def traversal(H, mode):
    return {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mode]


def check(tag, c, got, threshold, mode, batch):
    exp = G.expected(c, mode)
    ok = G.decidable(c, mode)
    with np.errstate(all="ignore"):
        err = np.max(np.abs(got - exp) / np.maximum(1.0, np.abs(exp)), axis=1)
    left_out = int((~ok & ~c["bad"]).sum()) + (int(c["bad"].sum()) if batch == "camera" else 0)
    print("%s: %d rays compared, %d fragile and %d badly conditioned left out; largest error %.3g of %.3g allowed"
          % (tag, int(ok.sum()), int((~ok & ~c["bad"]).sum()), int(c["bad"].sum()), float(np.max(err[ok], initial=0.0)), threshold))
    assert left_out <= G.FRAGILE_CAP[batch] * len(ok), "%s: too many rays left out as fragile" % tag
    assert batch == "camera" or int(c["bad"].sum()) <= G.REPLACED_CAP * dict(G.BATCHES)[batch], "%s: too many rays left out as badly conditioned" % tag
    bad = ok & ~G.agreement(exp, got, threshold)
    assert not bad.any(), "%s: %d rays disagree with the exact reference; %s" % (tag, int(bad.sum()), G.first_disagreement(c, exp, got, bad))


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape and np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


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
    r = host.Renderer(s["host"], traversal(H, mode), kd_depth=G.KD_DEPTH)
    got = r.radiance(c["o"], c["d"], background=c["bg"], seed=0, sample=0, stream_base=0, reorder=reorder)["rgb"]
    r.close()
    tag = "%s %s %s reorder=%d" % (scene, name, mode, reorder)
    check(tag, c, got, TOL[scene], mode, name)
    same_bits(got, oracle_bits(scene, name, mode), tag + " vs po_color_rays")   # so both orders give the same bits


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene,name", CASES)
def test_a_slice_with_its_stream_base_equals_that_slice(host, H, scenes, oracle_bits, scene, name, mode):
    s, c = scenes[scene], scenes[scene]["batches"][name]
    n = len(c["o"])
    k, m = n // 3, n // 2
    r = host.Renderer(s["host"], traversal(H, mode), kd_depth=G.KD_DEPTH)
    part = [r.radiance(c["o"][k:k + m].copy(), c["d"][k:k + m].copy(), background=c["bg"][k:k + m].copy(), stream_base=k, reorder=ro)["rgb"] for ro in (False, True)]
    r.close()
    for p in part:
        same_bits(p, oracle_bits(scene, name, mode)[k:k + m], "%s %s %s: the slice [%d, %d) with its stream base" % (scene, name, mode, k, k + m))


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", G.batches_of("hall"))
def test_radiance_with_every_recursion_frame_in_hbm(host, H, scenes, oracle_bits, monkeypatch, name, mode, reorder):
    """PORTRAYER_PARK=0 (read at every call): no parked frame stays in LDS."""
    c = scenes["hall"]["batches"][name]
    r = host.Renderer(scenes["hall"]["host"], traversal(H, mode), kd_depth=G.KD_DEPTH)
    monkeypatch.setenv("PORTRAYER_PARK", "0")
    in_hbm = r.radiance(c["o"], c["d"], background=c["bg"], reorder=reorder)["rgb"]
    monkeypatch.delenv("PORTRAYER_PARK")
    r.close()
    tag = "hall %s %s reorder=%d, frames in HBM" % (name, mode, reorder)
    check(tag, c, in_hbm, TOL["hall"], mode, name)
    same_bits(in_hbm, oracle_bits("hall", name, mode), tag + " vs po_color_rays (as with the youngest frame in LDS)")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", G.SCENES)
def test_render_is_the_exact_colour_of_the_eye_rays(host, H, scenes, scene, mode):
    c = scenes[scene]["batches"]["camera"]
    w, h = (int(x) for x in c["size"])
    assert w * h == len(c["o"]) <= 16 * 12
    r = host.Renderer(scenes[scene]["host"], traversal(H, mode), kd_depth=G.KD_DEPTH)
    _, linear, st = r.render(c["cam"], w, h, c["bg"].reshape(h, w, 3), samples=1, seed=0, sample_mode=H.SAMPLE_CENTRE)
    r.close()
    check("%s render %s" % (scene, mode), c, linear.reshape(-1, 3), TOL[scene], mode, "camera")
    v = st["kernel_variant"]
    kernel = "chain" if v & H.KERNEL_CHAIN else ("interpreter" if v & H.KERNEL_INTERPRETER else "line")
    assert kernel == KERNEL[scene], "%s %s ran the %s kernel (variant %d)" % (scene, mode, kernel, v)
