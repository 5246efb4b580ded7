"""The oracle's textures, normal maps and uv_trans against an exact-arithmetic reading of the reference (tests/exact_shade.py: _maps), on the fixtures
of tests/golden/exact_textures/ (tools/gen_exact_textures.py).

Five scenes whose materials carry textures, normal maps and the four uv_trans of the generator, each with a `camera`, a `random` and a `special` batch;
the special rays are constructed to land 2^-12 texels beside texel edges, cube-face borders, the sphere's seam and its to-top test, in coordinates that
go negative (where truncation is not floor) and above 1 (where the wrap is modulo w, not w - 1), and on triangles' corners and edges. On every ray the
exact reference can decide the oracle's colour lies within the scene's threshold (64 times the reference's own 53-bit deviation, tolerances.json), in all
three traversals. Apart from any tolerance, the texel the oracle fetches at a camera ray's hit is the texel the exact reference names, byte for byte.

The comparisons need numpy only. The tests that re-evaluate the exact reference need mpmath and skip without it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import gen_exact_shading as G  # noqa: E402
import gen_exact_textures as T  # noqa: E402
from scene_dsl import Camera, Material, Node, Scene, Sphere  # noqa: E402
from test_exact_shading import check_against_exact, oracle_colors  # noqa: E402

TOL = T.load_tolerances()
MODES = ("flat", "kd", "hier")
CASES = [(s, b) for s in T.SCENES for b in T.BATCH_NAMES]
_cache = {}


def batch(scene, name):
    if (scene, name) not in _cache:
        _cache[scene, name] = T.load(scene, name)
    return _cache[scene, name]


def all_batches():
    return {s: {b: batch(s, b) for b in T.BATCH_NAMES} for s in T.SCENES}


@pytest.fixture(scope="module")
def packed(oracle):
    out = {}
    for s in T.SCENES:
        scene = T.build_scene(s)
        ps = oracle.pack(scene)
        assert oracle.flatten(ps)["trans"].tobytes() == batch(s, "camera")["trans"].tobytes(), "%s is not the scene of the fixture" % s
        out[s] = (scene, ps)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene,name", CASES)
def test_oracle_colours_agree_with_the_exact_reference(oracle, packed, scene, name, mode):
    c = batch(scene, name)
    got = oracle_colors(oracle, packed[scene][1], c["o"], c["d"], c["bg"], mode)
    assert check_against_exact("%s %s %s" % (scene, name, mode), c, got, TOL[scene], mode) >= len(c["o"]) // 2


def pow_as_the_kernels(x, y):
    """pt_pow by the header the kernels compile, built for the host (tests/test_pow_exact.py)."""
    from portrayer_amd import _hip as H
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.full_like(x, y)
    port, libm = np.empty_like(x), np.empty_like(x)
    assert H.lib().pt_test_pow_host(x.size, x.ctypes.data_as(H._dp), y.ctypes.data_as(H._dp), port.ctypes.data_as(H._dp), libm.ctypes.data_as(H._dp)) == 0
    return port


def texel_colours(c):
    """The diffuse colour of the exact texel's bytes, (byte / 255) ^ 2.2, and the rays it stands for: a decidable, textured, non-reflective primary hit."""
    rgb, textured = T.texel_bytes(c)
    which = textured & G.decidable(c, "flat") & np.isin(c["kind"], (G.PLAIN, G.SPEC_EPS))
    return pow_as_the_kernels((rgb[which] / 255.0).ravel(), 2.2).reshape(-1, 3), which


@pytest.mark.parametrize("scene", T.SCENES)
def test_the_oracle_fetches_the_exact_texel(oracle, scene):
    """No tolerance: under ambient (1, 1, 1) and no lights a non-reflective hit's colour is its diffuse colour, the texel's."""
    c = batch(scene, "camera")
    ps = oracle.pack(T.build_scene(scene, lights=False))
    assert oracle.flatten(ps)["trans"].tobytes() == c["trans"].tobytes()
    exp, which = texel_colours(c)
    print("%s: %d of %d eye rays meet a textured, non-reflective surface" % (scene, int(which.sum()), len(which)))
    assert int(which.sum()) >= 48
    for mode in MODES:
        got = oracle_colors(oracle, ps, c["o"][which], c["d"][which], c["bg"][which], mode)
        wrong = np.flatnonzero(np.any(got.view(np.uint64) != exp.view(np.uint64), axis=1))
        assert wrong.size == 0, "%s %s: %d texels differ, first at ray %d: exact bytes %s give %s, the oracle has %s" % (
            scene, mode, wrong.size, int(np.flatnonzero(which)[wrong[0]]), T.texel_bytes(c)[0][which][wrong[0]].tolist(), exp[wrong[0]].tolist(), got[wrong[0]].tolist())


# ---- the oracle's own count of sphere lookups near a texel edge, cross-checked
@pytest.mark.parametrize("scene", T.SCENES)
def test_near_edge_counter_is_zero_where_the_exact_margins_say_so(oracle, packed, scene):
    """Every eye ray of the camera batches is decidable: no lookup of its tree lies within 2^-30 of a texel edge, so none lies within 4096 ulps."""
    c = batch(scene, "camera")
    assert not (c["fragile"] | c["bad"]).any()
    w, h = (int(x) for x in c["size"])
    st = oracle.render(packed[scene][1], list(c["cam"]), w, h, background=c["bg"].reshape(h, w, 3), samples=1).stats
    print("%s: %d sphere lookups, %d near an edge" % (scene, st["tex_sphere_lookups"], st["tex_sphere_near_edge"]))
    assert st["tex_sphere_near_edge"] == 0
    assert st["tex_sphere_lookups"] > 0 or scene == "tex_tris"


def test_near_edge_counter_sees_a_ray_on_an_edge():
    """One eye ray onto a textured sphere, its eye moved by bisection until two adjacent f64 positions fetch different texels: that lookup lies within a
    few ulps of a texel edge, and the oracle counts it. (It is fragile by construction: counted here, compared with nothing.)"""
    import oracle_lib
    tx = T.load_textures()
    scene = Scene(Node.group([Node.geo(Sphere(), Material(texture=tx["t2"]))]), [], (1.0, 1.0, 1.0))
    ps = oracle_lib.pack(scene)

    def look(x):
        r = oracle_lib.render(ps, Camera(eye=(x, 0.3, 5.0), center=(0.0, 0.0, 0.0)), 1, 1, background=np.zeros((1, 1, 3)), samples=1)
        return r.linear[0, 0].tobytes(), r.stats

    lo, hi = 0.2, 0.9
    a, b = look(lo)[0], look(hi)[0]
    assert a != b, "the two eyes see the same texel"
    while np.nextafter(lo, hi) < hi:
        mid = lo + (hi - lo) / 2
        if look(mid)[0] == a:
            lo = mid
        else:
            hi = mid
    for x in (lo, hi):
        st = look(x)[1]
        assert st["tex_sphere_lookups"] == 1 and st["tex_sphere_near_edge"] == 1, (x, st)


# ---- the fixtures themselves
@pytest.mark.parametrize("scene", T.SCENES)
def test_fixture_meets_the_input_conditions(scene):
    """The caps per batch (the left-out counts are printed), and every constructed ray reached what it was built for."""
    T.check_conditions(scene, {b: batch(scene, b) for b in T.BATCH_NAMES})


def test_every_branch_of_the_maps_is_covered_twenty_times():
    assert T.COVER_MIN == 20
    T.check_coverage(all_batches())


def test_tolerances_are_the_measured_deviations():
    assert (T.FRAGILE, T.SLACK, T.THRESHOLD_CAP, T.MAX_CASTS, T.ILL) == (2.0 ** -30, 64.0, 2.0 ** -24, 96, 2.0 ** -31)
    assert (T.FRAGILE_CAP, T.REPLACED_CAP) == (G.FRAGILE_CAP, G.REPLACED_CAP)
    tol = G.tolerances(all_batches())
    for s in T.SCENES:
        print("%s: deviation %.3g, threshold %.3g" % (s, tol[s]["deviation"], tol[s]["threshold"]))
        assert TOL[s] == tol[s]["threshold"] == T.SLACK * tol[s]["deviation"] and 0.0 < TOL[s] <= T.THRESHOLD_CAP


def test_the_textures_are_the_generators_and_small():
    made, kept = T.make_textures(), T.load_textures()
    assert sorted(made) == sorted(kept) and all(np.array_equal(made[k], kept[k].pixels) for k in made)
    assert kept["n0"].pixels[:, :, 2].min() >= 140 and kept["n1"].pixels[:, :, 2].min() < 128
    for k, t in kept.items():
        h, w = t.pixels.shape[:2]
        assert (w - 1) % 4 != 0 and (h - 1) % 3 != 0, k
    files = os.listdir(T.OUT)
    sizes = [os.path.getsize(os.path.join(T.OUT, f)) for f in files]
    assert max(sizes) < 64 * 1024 and sum(sizes) < 512 * 1024


def test_the_recorded_events_are_the_evaluators():
    pytest.importorskip("mpmath", reason="mpmath is needed to evaluate the exact reference")
    import exact_shade
    assert exact_shade.TEX_EVENTS == T.TEX_EVENTS and exact_shade.GAMMA == 2.2 and exact_shade.EPS_F64 == T.EPSILON


def test_generator_reproduces_a_batch_byte_for_byte():
    pytest.importorskip("mpmath", reason="mpmath is needed to re-evaluate the exact reference")
    scene, name = T.CHECK_BATCH
    cols = T.make_batch(scene, name, workers=min(8, os.cpu_count() or 1))
    with open(T.path(scene, name), "rb") as fh:
        assert G.npz_bytes({k: v for k, v in cols.items() if k in T.STORED}) == fh.read()


# ---- the evaluator: lookups worked by hand, independent of the scenes
def exact_plane(pixels, uv_trans, normals=None):
    pytest.importorskip("mpmath", reason="mpmath is needed to evaluate the exact reference")
    import exact_shade
    import oracle_lib
    from scene_dsl import Plane, Texture
    m = Material(texture=Texture(pixels), normals=None if normals is None else Texture(normals), uv_trans=uv_trans)
    scene = Scene(Node.group([Node.geo(Plane(), m)]), [], (1.0, 1.0, 1.0))
    return exact_shade.ExactScene(scene, oracle_lib.flatten(oracle_lib.pack(scene))["trans"])


def test_closed_form_truncation_wrap_and_the_third_row():
    """A 5 x 3 texture whose red byte is 10 * x + y on a unit plane (u = x + 1/2, v = z + 1/2), looked at from above."""
    px = np.zeros((3, 5, 3), dtype=np.uint8)
    for y in range(3):
        for x in range(5):
            px[y, x] = (10 * x + y, 0, 0)
    red = lambda ex, u, v: ex.color((u - 0.5, 1.0, v - 0.5), (0.0, -1.0, 0.0), (0, 0, 0)).tex0["texel"][:3]
    ex = exact_plane(px, T.U_ID)
    assert red(ex, 0.3, 0.3) == (1, 0, 10)                  # trunc(0.3 * 4) = 1, trunc(0.3 * 2) = 0
    assert red(ex, 0.99, 0.99) == (3, 1, 31)                # the last column and row are reached at u = v = 1 only
    shifted = exact_plane(px, (1.0, 0.0, -0.2, 0.0, 1.0, -0.3, 0.0, 0.0, 1.0))
    assert red(shifted, 0.1, 0.1) == (0, 0, 0)              # -0.1 * 4 = -0.4 and -0.2 * 2 = -0.4 truncate to 0: not floored to the far edge
    assert red(shifted, 0.1, 0.9)[:2] == (0, 1)
    grown = exact_plane(px, (1.5, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 1.0))
    assert red(grown, 0.7, 0.6)[:2] == (4, 2)               # 1.05 * 4 = 4.2 -> 4 (modulo 5, not 4); 1.2 * 2 = 2.4 -> 2
    assert red(grown, 0.9, 0.8)[:2] == (0, 0)               # 1.35 * 4 = 5.4 -> 5 -> 0; 1.6 * 2 = 3.2 -> 3 -> 0
    row3 = exact_plane(px, (1.5, 0.0, 0.0, 0.0, 2.0, 0.0, 7.0, -3.0, 0.25))
    assert red(row3, 0.7, 0.6) == red(grown, 0.7, 0.6)      # the third row is computed and dropped
    s = ex.color((-0.2, 1.0, -0.2), (0.0, -1.0, 0.0), (0, 0, 0))
    assert s.rgb() == pytest.approx([(10 / 255.0) ** 2.2, 0.0, 0.0], rel=1e-15)
    on_edge = ex.color((0.0, 1.0, 0.1), (0.0, -1.0, 0.0), (0, 0, 0))   # u = 1/2: 0.5 * 4 is the integer 2
    assert on_edge.margin == 0.0


def test_closed_form_normal_map_on_a_plane():
    """normal_at: (r, g, b) -> (2r - 1, 2g - 1, -(2b - 1)) -> (nx, -nz, -ny); the plane's basis is the identity; normalised before the basis only."""
    px = np.full((2, 2, 3), 128, dtype=np.uint8)
    nm = np.zeros((2, 2, 3), dtype=np.uint8)
    nm[:, :] = (255, 0, 255)   # (1, -1, -1) -> (1, 1, 1) -> normalised
    ex = exact_plane(px, T.U_ID, nm)
    import exact_shade
    from mpmath import mp, mpf
    with mp.workprec(256):
        h = ex.cast((0.1, 1.0, 0.1), (0.0, -1.0, 0.0))
        st = exact_shade._Tree(None, 10)
        normal, _ = exact_shade._maps(ex, st, h, ex.shading()["materials"][0], (mpf(0), mpf(1), mpf(0)), 0)
        assert [float(x) for x in normal] == pytest.approx([3 ** -0.5] * 3, rel=1e-15)
