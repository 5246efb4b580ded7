"""Every <MODE family, TEX, PARK> cell of the shading passes that make or read their own rays - film, film_map, lens, gather, probe - against pt_radiance along
that pass's contract rays, bit for bit: what the passes share is their frame (csrc/pt_shade_frame.h), and this file is where a change of it shows in every
instantiation family at once. pt_radiance itself stays pinned to the oracle by tests/test_gpu_radiance.py.

Cells: {film, film_map, lens, gather, probe} x {flat, kd, hier} x {TEX 0, 1} x {PARK 0, 1}. TEX is the scene's: one scene with a material map, one without,
the same geometry otherwise; both hold a dielectric, so the passes park their youngest frame in LDS (PARK 1). PARK 0 is PORTRAYER_PARK=0, set for a child
process that runs this file's cells as a script. The scene properties relied on are asserted.

Rays and order per pass:
  film, film_map   the camera ray through the pixel centre (the oracle's camera, as tests/test_gpu_radiance.py makes it), sample s, stream y * W + x, the pixel's
                   background; a pixel's samples folded by pt_test_film_fold_host and divided as resolve divides
  lens             pt_test_lens_rays_host's rays of a thin lens with an aperture, jittered; folded the same way
  gather           pt_test_ao_rays_host's rays, stream first_index * S + q * S + k; a point's S colours added per channel from zero in ascending k
  probe            pt_test_probe_host's rays and basis values; per round of 64 from zero in ascending k, the rounds left to right (probe_restate.project)
Shapes: a 16 x 8 film with 3 samples (K = 4: an idle lane per pixel); a budget map over {0, 1, 2, 3} whose list ends inside a wavefront; 5 points at 16 samples
(the second wavefront runs past n) with one invalid; 2 probes and an invalid one at 128 directions (two rounds). Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from lens_restate import replay as lens_replay  # noqa: E402
from probe_restate import project  # noqa: E402
from test_ao_contract import replay as ao_replay  # noqa: E402
from test_probe_contract import replay as probe_replay  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HT = 16, 8
SAMPLES = 3
SEED = 7
BG = (0.25, 0.5, 1.0)
PASSES = ("film", "film_map", "lens", "gather", "probe")
TRAVERSALS = ("flat", "kd", "hier")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def glass_scene(textured):
    """The water glass of tests/example_scenes.py with an area light; its wall and table carry their maps or, untextured, a plain colour."""
    from example_scenes import ASSETS
    from scene_dsl import Camera, Cube, Cylinder, Light, Material, Node, Plane, Scene, Texture, to_radians
    tex = lambda name: Texture.open(os.path.join(ASSETS, name)) if textured else None
    mat_wall = Material(diffuse=(0.6, 0.3, 0.2), specular=(0.3, 0.3, 0.3), shininess=25.0, texture=tex("Brick_Wall_013_COLOR.jpg"), normals=tex("Brick_Wall_013_NORM.jpg"))
    mat_table = Material(diffuse=(0.4, 0.3, 0.1), specular=(0.5, 0.5, 0.5), shininess=100.0, reflectivity=0.2, glossy_side_length=2.0,
                         texture=tex("Wood_018_basecolor_cubemap.jpg"), normals=tex("Wood_018_normal_cubemap.jpg"))
    mat_water = Material(diffuse=(0.0, 0.0, 0.1), specular=(0.3, 0.3, 0.3), shininess=25.0, reflectivity=0.9, refraction_index=1.33)
    mat_straw = Material(diffuse=(0.8, 0.0, 0.0), specular=(0.3, 0.3, 0.3), shininess=25.0)
    room = Node.group([Node.geo(Plane(), mat_wall).scaled(10.0).rotated_x(to_radians(90.0)).translated((0.0, 1.0, -2.0)),
                       Node.geo(Cube(), mat_table).scaled((8.0, 0.4, 4.0)).translated((0.0, 0.0, -0.2))])
    drink = Node.group([Node.geo(Cylinder(), mat_water).scaled((1.0, 1.4, 1.0)).translated((0.0, 0.7, 0.0)),
                        Node.geo(Cylinder(), mat_straw).scaled((0.1, 2.0, 0.1)).rotated_z(to_radians(28.4282)).translated((-0.165556, 0.911109, 0.1))]).translated((0.0, 0.2, 0.0))
    lights = [Light(position=(0.0, 27.0, 5.0), color=(0.5, 0.5, 0.5)), Light(position=(3.0, 6.0, 6.0), color=(0.25, 0.25, 0.25), area_a=(0.0, 0.5, 0.0), area_b=(0.5, 0.0, 0.0))]
    return Scene(root=Node.group([room, drink]), lights=lights, ambient=(0.3, 0.3, 0.3)), Camera(eye=(0.0, 3.2, 7.151111), center=(0.0, 0.091525, -5.719519), fovy_degrees=23.0)


_CASES = {}


def case(O, tex, mname):
    """A renderer of the scene in one traversal and what every cell of it shares: made once, never written to."""
    from portrayer_amd import _hip as H
    from portrayer_amd import host
    key = (tex, mname)
    if key in _CASES:
        return _CASES[key]
    scene, cam = glass_scene(bool(tex))
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    ex = hs.export()
    assert ("n_textures" in ex) == bool(tex), "TEX is chosen by whether the scene has a material map"
    assert (ex["materials"][:, 9] > 0.0).any(), "PARK = 1 wants a scene whose hits spawn rays: a dielectric"
    r = host.Renderer(hs, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mname], kd_depth=8)
    bg = np.random.default_rng(3).uniform(0.0, 1.0, size=(HT, W, 3))
    ys, xs = np.mgrid[0:HT, 0:W]
    # the film's samples: radiance along the pixel-centre camera rays, sample s, the pixel's stream and background
    o, d = O.camera_rays(cam, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    centre = np.stack([r.radiance(o, d, background=bg.reshape(-1, 3), seed=SEED, sample=s, stream_base=0)["rgb"] for s in range(SAMPLES)])
    # the lens film's: the contract's rays, jittered
    focus = float(np.linalg.norm(c10[3:6] - c10[0:3]))
    lens = host.Lens.thin(0.04 * focus, focus)
    l, pc = lens.struct(), host.camera(c10, W, HT)
    xy = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)
    behind = []
    for s in range(SAMPLES):
        lo, ld = lens_replay(H, pc, (l.model, l.aperture, l.focus, l.extent), W, HT, SEED, H.SAMPLE_RNG, xy, np.full(len(xy), s, dtype=np.uint32))
        behind.append(r.radiance(lo, ld, background=bg.reshape(-1, 3), seed=SEED, sample=s, stream_base=0)["rgb"])
    # points for gather and probe: what the camera sees, four of them and one that is invalid
    aov = r.aov(c10, W, HT, want=("position", "normal", "node"))
    hit = np.flatnonzero(aov["node"].ravel() >= 0)
    assert len(hit) >= 8
    take = hit[np.linspace(0, len(hit) - 1, 5).astype(int)]
    P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)[take]), np.ascontiguousarray(aov["normal"].reshape(-1, 3)[take])
    N[2] = 0.0  # no normal: an invalid point inside the first wavefront
    probes = np.ascontiguousarray(P[[0, 2, 4]] + 0.25 * aov["normal"].reshape(-1, 3)[take][[0, 2, 4]])
    probes[1, 1] = np.nan  # an invalid probe between two valid ones
    c = dict(r=r, c10=c10, bg=bg, centre=centre, behind=np.stack(behind), lens=lens, P=P, N=N, probes=probes, eye=np.array(list(pc.eye)))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[key] = c
    return c


def folded(H, samples, counts):
    """Per pixel p the fold of its first counts[p] samples (samples: (n, pixels, 3)) divided as resolve divides; pixels without samples are NaN."""
    out = np.full((samples.shape[1], 3), np.nan)
    for p, n in enumerate(counts):
        if n:
            one, total = np.ascontiguousarray(samples[:n, p, :]), np.zeros(3)
            assert H.lib().pt_test_film_fold_host(int(n), one.ctypes.data_as(H._dp), (C.c_uint32 * 1)(int(n)), 1, total.ctypes.data_as(H._dp)) == H.OK
            out[p] = total / float(n)
    return out


def film_cell(H, c, which):
    film = c["r"].film(W, HT)
    counts = np.full(HT * W, SAMPLES, dtype=np.uint32)
    if which == "film":
        film.add(c["c10"], c["bg"], samples=SAMPLES, seed=SEED, sample_mode=H.SAMPLE_CENTRE)
    elif which == "lens":
        film.add(c["c10"], c["bg"], samples=SAMPLES, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=c["lens"])
    else:
        counts = np.random.default_rng(5).integers(0, SAMPLES + 1, size=HT * W).astype(np.uint32)
        assert len(np.unique(counts)) == SAMPLES + 1 and int(counts.sum()) % 64 != 0 and int(counts.sum()) > 64, "unequal counts, and a list that ends inside a wavefront"
        film.add_map(c["c10"], c["bg"], counts.reshape(HT, W), seed=SEED, sample_mode=H.SAMPLE_CENTRE)
    assert np.array_equal(film.counts().ravel(), counts)
    linear = np.full((HT, W, 3), np.nan)
    film.resolve(linear_into=linear)
    film.close()
    want = folded(H, c["behind"] if which == "lens" else c["centre"], counts)
    assert np.array_equal(bits(linear.reshape(-1, 3)), bits(want)), "%d values differ" % int((bits(linear.reshape(-1, 3)) != bits(want)).sum())
    seen = (bits(want[counts > 0]) != bits(c["bg"].reshape(-1, 3)[counts > 0])).any(axis=1)
    assert seen.any(), "the film sees the scene"


def gather_cell(H, c):
    S, first = 16, 3
    O, D, valid = ao_replay(H, c["P"], c["N"], S, seed=SEED, pas=1, first=first, eye=c["eye"])
    assert valid.tolist() == [1, 1, 0, 1, 1]
    O[valid == 0], D[valid == 0] = 0.0, 0.0  # (an invalid point has no rays: these are not traced and not read)
    rgb = c["r"].radiance(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), BG, seed=SEED, sample=1, stream_base=first * S)["rgb"].reshape(5, S, 3)
    total = np.zeros((5, 3))
    for k in range(S):
        total = total + rgb[:, k, :]
    total[valid == 0] = 0.0
    got = c["r"].gather(c["P"], c["N"], BG, samples=S, seed=SEED, pass_index=1, first_index=first, eye=c["eye"], want=("sum", "valid"))
    assert np.array_equal(got["valid"], valid.astype(np.uint8))
    assert np.array_equal(bits(got["sum"]), bits(total)), "%d values differ" % int((bits(got["sum"]) != bits(total)).sum())
    assert (total[valid == 1] != np.array(BG) * S).any(), "some ray meets the scene"


def probe_cell(H, c):
    S, first = 128, 2
    O, D, Y, valid = probe_replay(H, c["probes"], S, seed=SEED, pas=1, first=first)
    assert valid.tolist() == [1, 0, 1]
    O[valid == 0], D[valid == 0] = 0.0, 0.0
    rgb = c["r"].radiance(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), BG, seed=SEED, sample=1, stream_base=first * S)["rgb"].reshape(3, S, 3)
    want = project(Y, rgb, valid)
    got = c["r"].probe(c["probes"], BG, samples=S, seed=SEED, pass_index=1, first_index=first, want=("sh", "valid"))
    assert np.array_equal(got["valid"], valid.astype(np.uint8))
    assert np.array_equal(bits(got["sh"]), bits(want)), "%d values differ" % int((bits(got["sh"]) != bits(want)).sum())
    assert not np.array_equal(bits(want), bits(project(Y, np.broadcast_to(np.array(BG), rgb.shape), valid))), "some ray meets the scene"


def cell(O, which, mname, tex):
    from portrayer_amd import _hip as H
    c = case(O, tex, mname)
    if which == "gather":
        gather_cell(H, c)
    elif which == "probe":
        probe_cell(H, c)
    else:
        film_cell(H, c, which)


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for c in _CASES.values():
        c["r"].close()
    _CASES.clear()


@pytest.mark.parametrize("tex", [0, 1])
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", PASSES)
def test_a_pass_has_the_bits_of_radiance_along_its_rays_with_frames_parked_in_lds(oracle, which, mname, tex):
    assert os.environ.get("PORTRAYER_PARK", "1") != "0", "PARK = 1 is the scene's choice: nothing may switch it off here"
    cell(oracle, which, mname, tex)


@pytest.mark.parametrize("tex", [0, 1])
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_the_five_passes_with_every_parked_frame_in_hbm(oracle, mname, tex):
    """PARK = 0: PORTRAYER_PARK=0 from the start of a process of its own, which runs the five cells of this traversal and scene."""
    env = dict(os.environ, PORTRAYER_PARK="0")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), mname, str(tex)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert done.returncode == 0 and "shade frame cells ok: " + " ".join(PASSES) in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import oracle_lib
    oracle_lib.build()
    assert os.environ.get("PORTRAYER_PARK") == "0"
    for name in PASSES:
        cell(oracle_lib, name, sys.argv[1], int(sys.argv[2]))
    for c in _CASES.values():
        c["r"].close()
    print("shade frame cells ok: " + " ".join(PASSES))
