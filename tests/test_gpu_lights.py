"""Shadow rays at 0 to 65 lights, against the oracle. The kernels branch on the light count where no scene of the other tests reaches:
the interpreter handles lights in rounds of PT_LIGHT_ROUND = 32 (a 32-bit mask of shadow results per round, the colour parked between
rounds, the area-light draw counter restarted per round; pt_shade.h), scenes of more than 32 lights keep recursion frames in HBM and get
one stream for both slots (pt_context.h: pt_needs_spill; pt_api.hip: pt_context_stream), fork / join is off above 32 lights, and the occluder table holds
one word per (tile, light) and is left out above 4 MB. 0, 1, 31, 32, 33, 64 and 65 lights are the round boundaries (65: three rounds, the
last with one light), in each kernel family - straight-line (nothing reflective, and a 1000-node scene for the 4- to 6-wave
instantiations), chain (opaque mirrors, one glossy) and interpreter (a dielectric) - x flat / k-d / hierarchical semantics, counting and
plain instantiation: u8 pixels, f64 means and ray counts."""
import os

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cube, Cylinder, Light, Material, Node, Plane, Scene, Sphere, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 31, 32, 33, 64, 65]
KINDS = ["plain", "mirror", "glass", "big"]  # big: big-scene's 1000 nodes with its lights replaced (nothing reflective)
MODES = ["flat", "kd", "hier"]
W, H_ = 37, 23
ENV = ("PORTRAYER_WAVES", "PORTRAYER_KD_WAVES", "PORTRAYER_CHAIN_WAVES", "PORTRAYER_CHAIN", "PORTRAYER_FORK", "PORTRAYER_PARK",
       "PORTRAYER_SHADOW_CACHE", "PORTRAYER_OCC_SEED", "PORTRAYER_TWO_STREAMS")

_SPHERE3 = (0.0, 2.5, -3.0)  # the centre of the floating sphere: lights placed there are always blocked


def _lights(n, seed, area=True, spread=8.0, height=(3.0, 12.0), below=-2.0, inside=_SPHERE3, area_size=0.6, falloffs=None):
    """n lights, placed deterministically: about every third an area light, falloffs varying, every seventh from the fourth below the
    floor and every seventh from the sixth inside an occluder (always blocked), lights 0 and 1 at one position."""
    rng = np.random.default_rng(9100 + 131 * n + seed)
    falloffs = falloffs or [(1.0, 0.0, 0.0), (1.0, 0.02, 0.001), (0.6, 0.05, 0.004)]
    out = []
    for i in range(n):
        pos = (float(rng.uniform(-spread, spread)), float(rng.uniform(*height)), float(rng.uniform(-spread, spread)))
        if i % 7 == 3 and below is not None:
            pos = (pos[0] * 0.3, below, pos[2] * 0.3)
        elif i % 7 == 5:
            pos = tuple(float(c) + 0.01 * float(rng.uniform(-1, 1)) for c in inside)
        elif i == 1:
            pos = out[0].position
        color = tuple(float(c) for c in rng.uniform(0.3, 1.0, 3) * 1.6 / (n + 1))
        is_area = area and i % 3 == 2
        out.append(Light(position=pos, color=color, falloff=falloffs[(i // 2) % len(falloffs)],
                         area_a=(area_size, 0.0, 0.0) if is_area else (0.0, 0.0, 0.0), area_b=(0.0, 0.0, area_size) if is_area else (0.0, 0.0, 0.0)))
    return out


def lit_scene(n_lights, kind, seed=0, area=True):
    """A floor, three spheres, a rotated cube under a transformed group and a cylinder under n_lights lights (_lights). kind: plain (nothing
    reflective: the straight-line kernels), mirror (opaque reflective materials, one glossy: the chain kernel), glass (a dielectric: the
    interpreter), big (big-scene's 1000 primitives under n_lights lights: the 4- to 6-wave straight-line instantiations)."""
    if kind == "big":
        from example_scenes import EXAMPLES
        scene, cam, _ = EXAMPLES["big-scene"]()
        inside = scene.root.children[555].ops[-1][1]  # (the translation of one of its primitives)
        scene.lights = _lights(n_lights, seed, area, spread=600.0, height=(-400.0, 600.0), below=None, inside=inside, area_size=40.0,
                               falloffs=[(1.0, 0.0, 0.0), (1.0, 0.001, 0.0), (0.8, 0.0, 1e-6)])
        return scene, cam
    floor = Material(diffuse=(0.7, 0.7, 0.6), specular=(0.2, 0.2, 0.2), shininess=10.0)
    red = Material(diffuse=(0.8, 0.2, 0.2), specular=(0.5, 0.5, 0.5), shininess=40.0)
    blue = Material(diffuse=(0.2, 0.3, 0.8), specular=(0.3, 0.3, 0.3), shininess=25.0)
    green = Material(diffuse=(0.2, 0.7, 0.3), specular=(0.4, 0.4, 0.4), shininess=60.0)
    if kind == "mirror":
        blue = Material(diffuse=(0.1, 0.1, 0.2), specular=(0.8, 0.8, 0.8), shininess=200.0, reflectivity=0.6)
        green = Material(diffuse=(0.2, 0.5, 0.3), specular=(0.3, 0.3, 0.3), shininess=100.0, reflectivity=0.4, glossy_side_length=0.3)
    elif kind == "glass":
        blue = Material(diffuse=(0.0, 0.0, 0.05), specular=(0.3, 0.3, 0.3), shininess=25.0, reflectivity=0.9, refraction_index=1.5)
    kids = [Node.geo(Plane(), floor).scaled(30.0),
            Node.geo(Sphere(), red).scaled(0.8).translated((-2.0, 1.0, -1.0)),
            Node.geo(Sphere(), blue).scaled(0.7).translated((1.5, 0.7, 1.5)),
            Node.geo(Sphere(), red).translated(_SPHERE3),
            Node.group([Node.geo(Cube(), green).scaled((0.6, 1.8, 0.6)).rotated_y(0.5)]).rotated_x(0.2).translated((2.5, 0.3, -1.5)),
            Node.geo(Cylinder(), floor).scaled((0.5, 1.5, 0.5)).translated((-1.0, 0.75, 2.0))]
    scene = Scene(root=Node.group(kids), lights=_lights(n_lights, seed, area), ambient=(0.1, 0.1, 0.1))
    return scene, Camera(eye=(0.5, 5.0, 10.0), center=(0.0, 0.5, 0.0), fovy_degrees=45.0)


def family(H, v):
    """The kernel family a render's kernel_variant names."""
    if v & H.KERNEL_CHAIN:
        return "chain"
    if v & H.KERNEL_INTERPRETER:
        return "fork" if v & H.KERNEL_FORK else ("park" if v & H.KERNEL_PARK else "interp")
    return "line"


_SCENES = {}  # (n, kind, point_only) -> (oracle's packed scene, camera, host scene)
_ORACLE = {}  # (n, kind, point_only, mode, w, h, samples) -> oracle render: the same for every switch


def _scene(n, kind, point_only=False):
    key = (n, kind, point_only)
    if key not in _SCENES:
        import oracle_lib
        scene, cam = lit_scene(n, kind, area=not point_only)
        _SCENES[key] = (oracle_lib.pack(scene), cam, host_glue.host_scene(scene))
    return _SCENES[key]


def _traverse(H, oracle, mode):
    return {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]


def _reference(oracle, n, kind, mode, w, h, samples, point_only=False):
    key = (n, kind, point_only, mode, w, h, samples)
    if key not in _ORACLE:
        scene, cam, _ = _scene(n, kind, point_only)
        om = {"flat": oracle.MODE_FLAT, "kd": oracle.MODE_KD, "hier": oracle.MODE_HIER}[mode]
        _ORACLE[key] = oracle.render(scene, cam, w, h, samples=samples, seed=5, jitter=oracle.JITTER_RNG, mode=om, kd_depth=8)
    return _ORACLE[key]


def _log_variant(n, kind, mode, switch, variant):
    log = os.environ.get("PT_VARIANT_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{n} {kind} {mode} {switch or '-'} {variant}\n")


def render_and_compare(H, oracle, n, kind, mode, w, h, samples, switch="", point_only=False):
    """Counting and plain render of (n, kind) against the oracle; returns the two kernel variants."""
    from portrayer_amd import host
    scene, cam, hs = _scene(n, kind, point_only)
    ref = _reference(oracle, n, kind, mode, w, h, samples, point_only)
    r = host.Renderer(hs, _traverse(H, oracle, mode)[0], kd_depth=8)
    kw = dict(samples=samples, seed=5, sample_mode=H.SAMPLE_RNG)
    bg = default_background(w, h)
    c10 = host_glue.cam10(cam)
    rgb, lin, st = r.render(c10, w, h, bg, stats=True, **kw)
    plain, plain_lin, st0 = r.render(c10, w, h, bg, **kw)
    r.close()
    where = f"{n} lights, {kind}, {mode}, {w}x{h}x{samples} {switch}: variant {st['kernel_variant']} / {st0['kernel_variant']}"
    assert st["kernel_variant"] & H.KERNEL_COUNTING and not st0["kernel_variant"] & H.KERNEL_COUNTING, where
    assert st["kernel_variant"] & ~H.KERNEL_COUNTING == st0["kernel_variant"], where
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], (where, k)
    assert np.array_equal(rgb, ref.rgb), f"{where}: {(rgb != ref.rgb).any(axis=2).sum()} pixels differ"
    assert np.array_equal(plain, ref.rgb), f"{where}: plain: {(plain != ref.rgb).any(axis=2).sum()} pixels differ"
    assert_ulp(lin, ref.linear, 0, where)
    assert_ulp(plain_lin, ref.linear, 0, where + " (plain)")
    if n > 0:
        assert ref.stats["shadow"] > 0, where
    _log_variant(n, kind, mode, switch, st0["kernel_variant"])
    return st["kernel_variant"], st0["kernel_variant"]


EXPECTED = {"plain": "line", "big": "line", "mirror": "chain", "glass": "park"}


@pytest.fixture
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def test_the_oracle_takes_an_empty_light_list(oracle):
    scene, cam = lit_scene(0, "plain")
    ref = oracle.render(scene, cam, 9, 7, samples=1, seed=5, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert ref.stats["shadow"] == 0 and ref.stats["hits"] > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", COUNTS)
def test_light_count_against_the_oracle(H, oracle, clean_env, n, kind, mode):
    samples = (1, 3, 8)[(COUNTS.index(n) + KINDS.index(kind) + MODES.index(mode)) % 3]
    _, v = render_and_compare(H, oracle, n, kind, mode, W, H_, samples)
    assert family(H, v) == EXPECTED[kind], (n, kind, mode, v)
    if kind == "big" and mode != "kd":
        assert v & H.KERNEL_WAVES_MASK == 6, v  # (the densest straight-line instantiation: mesh-free, >= 256 nodes)


@pytest.mark.parametrize("kind", ["glass", "mirror"])
def test_65_lights_at_64_samples(H, oracle, clean_env, kind):
    """A wavefront = one pixel's 64 samples: every lane in the same rounds of lights."""
    _, v = render_and_compare(H, oracle, 65, kind, "hier", 11, 7, 64)
    assert family(H, v) == EXPECTED[kind]


# switch -> (kinds, the family the switch makes them run, the waves it asks for (None: not checked), semantics it acts in)
SWITCHES = {
    "PORTRAYER_PARK=0": (["mirror", "glass"], "interp", None, MODES),  # (pt_api.hip: without a parked frame the chain kernel is not taken either)
    "PORTRAYER_CHAIN=0": (["mirror"], "park", None, MODES),
    "PORTRAYER_WAVES=3": (["plain", "big"], "line", 3, ["flat", "hier"]),
    "PORTRAYER_WAVES=4": (["plain", "big"], "line", 4, ["flat", "hier"]),
    "PORTRAYER_WAVES=5": (["plain", "big"], "line", None, ["flat", "hier"]),
    "PORTRAYER_KD_WAVES=3": (["big"], "line", 3, ["kd"]),
    "PORTRAYER_KD_WAVES=4": (["big"], "line", 4, ["kd"]),
    "PORTRAYER_CHAIN_WAVES=3": (["mirror"], "chain", 3, MODES),
}


@pytest.mark.parametrize("n", [32, 33, 65])
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switches_at_the_round_boundaries(H, oracle, clean_env, switch, n):
    kinds, fam, waves, modes = SWITCHES[switch]
    k, v = switch.split("=")
    clean_env.setenv(k, v)
    for kind in kinds:
        for mode in modes:
            _, var = render_and_compare(H, oracle, n, kind, mode, W, H_, 3, switch=switch)
            assert family(H, var) == fam, (switch, n, kind, mode, var)
            if waves is not None:
                assert var & H.KERNEL_WAVES_MASK == waves, (switch, n, kind, mode, var)


@pytest.mark.parametrize("n", [32, 33])
def test_fork_up_to_32_lights(H, oracle, clean_env, n):
    """PORTRAYER_FORK=1 on a dielectric scene lit by point lights only: fork / join up to PT_LIGHT_ROUND lights, the parked interpreter above."""
    clean_env.setenv("PORTRAYER_FORK", "1")
    for mode in MODES:
        _, v = render_and_compare(H, oracle, n, "glass", mode, W, H_, 3, switch="PORTRAYER_FORK=1", point_only=True)
        assert family(H, v) == ("fork" if n <= 32 else "park"), (n, mode, v)


@pytest.mark.parametrize("mode", ["flat", "hier"])
def test_occluder_table_cutoff_at_4_mb(H, oracle, clean_env, capfd, mode):
    """65 lights, one sample: 1016 x 1016 (16,129 tiles, 4,193,540 bytes: the table is kept) and 1024 x 1024 (16,384 tiles, 4,259,840 bytes:
    left out) - with and without the table (PORTRAYER_SHADOW_CACHE=0) the same images and f64 means, and a slice that does not start at 0.
    Whether the table exists is read from the seeding hook's line (PORTRAYER_VERBOSE=1)."""
    from portrayer_amd import host
    _, _, hs = _scene(65, "big")
    cam = host_glue.cam10(_scene(65, "big")[1])
    r = host.Renderer(hs, _traverse(H, oracle, mode)[0])
    for size, rect, table in ((1016, None, True), (1024, None, False), (1016, (13, 7, 1000, 1010), True)):
        bg = default_background(size, size)
        kw = dict(samples=1, seed=2, sample_mode=H.SAMPLE_RNG, rect=rect)
        clean_env.delenv("PORTRAYER_SHADOW_CACHE", raising=False)
        clean_env.setenv("PORTRAYER_VERBOSE", "1")
        clean_env.setenv("PORTRAYER_OCC_SEED", "0")  # (all entries "none": what the zeroed table holds)
        capfd.readouterr()
        rgb, lin, st = r.render(cam, size, size, bg, into=np.full((size, size, 3), 7, dtype=np.uint8), **kw)
        seeded = [l for l in capfd.readouterr().err.splitlines() if "occluder table" in l]
        clean_env.delenv("PORTRAYER_VERBOSE")
        clean_env.delenv("PORTRAYER_OCC_SEED")
        assert len(seeded) == (1 if table else 0), (size, rect, seeded)
        if table and rect is None:
            assert seeded[0] == f"[pt_render] occluder table: {(size // 8) ** 2 * 65} entries seeded (PORTRAYER_OCC_SEED=0)", seeded
        on, lin_on, _ = r.render(cam, size, size, bg, into=np.full((size, size, 3), 7, dtype=np.uint8), **kw)
        clean_env.setenv("PORTRAYER_SHADOW_CACHE", "0")
        off, lin_off, _ = r.render(cam, size, size, bg, into=np.full((size, size, 3), 7, dtype=np.uint8), **kw)
        assert st["kernel_mode"] == (6 if mode == "hier" else 3)
        for img, l in ((rgb, lin), (on, lin_on)):
            assert np.array_equal(img, off), f"{size} {rect}: {(img != off).any(axis=2).sum()} pixels differ"
            assert_ulp(l, lin_off, 0)
    r.close()
