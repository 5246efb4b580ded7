"""The film (pt_film_* / Renderer.film): samples accumulate on the device, and what resolve() gives at a pixel carries the bits of a render with that pixel's
count of samples - however the samples were split over adds and slices, in all three traversals.

Every comparison in this file is exact: bits() equality of f64 and equality of u8. Nothing is left out of a comparison except, for the ORACLE comparison only,
renders in which the oracle counts a sphere texture coordinate near a texel edge (tests/test_gpu_textures.py: texel_edge_proof), which can happen only in
scenes that texture or normal-map a sphere; the comparison with pt_render is unconditional."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import default_background  # noqa: E402
from test_gpu_aov import bits, modes  # noqa: E402
from test_gpu_radiance import all_examples, example_names  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37  # a multiple of 8 in neither direction
SPHERE = 0  # PT_PRIM_SPHERE
ADDS = (3, 5, 9, 1)  # 3 | 8 | 17 | 18: the second and third add cross a chunk boundary, the second ends on one


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def same_image(got, want, what):
    """(rgb, linear) against (rgb, linear): u8 equal, f64 equal in their bits."""
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "%s: rgb differs at %d pixels" % (what, int((got[0] != want[0]).any(axis=2).sum()))
    a, b = bits(got[1]), bits(want[1])
    assert a.shape == b.shape and np.array_equal(a, b), "%s: linear differs in %d of %d values" % (what, int((a != b).sum()), a.size)


def maps_a_sphere(hs):
    """Some node that carries a textured or normal-mapped material is a sphere: the only scenes whose texture coordinates go through atan2 / acos."""
    a = hs.export()
    mapped = [m for m in range(len(a["material_texture"])) if a["material_texture"][m] >= 0 or a["material_normal_map"][m] >= 0]
    prim, mat = np.asarray(a["prim_type"]), np.asarray(a["material"])
    return bool((np.isin(mat, mapped) & (prim == SPHERE)).any())


# ---- 1. every example scene: the film after each add == pt_render == the oracle
@pytest.mark.parametrize("name", example_names())
def test_every_add_leaves_the_render_of_the_samples_so_far(oracle, host, H, name):
    scene, cam, _ = all_examples()[name]()
    ps = oracle.pack(scene)
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(sum(map(ord, name))).uniform(0.0, 1.0, size=(HT, W, 3))
    compared, skipped = 0, 0
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        total = 0
        for n in ADDS:
            film.add(c10, bg, samples=n, seed=7, sample_mode=H.SAMPLE_RNG)
            total += n
            got = film.resolve()
            assert np.all(film.counts() == total)
            rgb, linear, _ = r.render(c10, W, HT, bg, samples=total, seed=7, sample_mode=H.SAMPLE_RNG)
            same_image(got, (rgb, linear), f"{name} {mname} {total} samples: film vs pt_render")
            ref = oracle.render(ps, cam, W, HT, background=bg, samples=total, seed=7, jitter=oracle.JITTER_RNG, mode=om, kd_depth=8)
            if ref.stats["tex_sphere_near_edge"] != 0:
                skipped += 1
                continue
            same_image(got, (ref.rgb, ref.linear), f"{name} {mname} {total} samples: film vs the oracle")
            compared += 1
        film.close()
        r.close()
    assert total == 18
    assert skipped == 0 or maps_a_sphere(hs), f"{name}: {skipped} oracle comparisons skipped in a scene that maps no sphere"
    assert compared + skipped == 3 * len(ADDS) and (compared == 3 * len(ADDS) or maps_a_sphere(hs))


# ---- 2. one add == four adds
@pytest.mark.parametrize("name", ["glossy-reflection", "soft-shadows", "entering-the-mirror-dimension", "transmission-refraction"])
def test_one_add_of_18_equals_the_four_adds(oracle, host, H, monkeypatch, name):
    """Draws (glossy material, area light), the chain and dielectrics. Film state against film state, through resolve and counts. The mirror scene parks
    recursion frames: there the four adds run once more with every parked frame in HBM (PORTRAYER_PARK=0)."""
    scene, cam, _ = all_examples()[name]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(5).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        one, four = r.film(W, HT), r.film(W, HT)
        one.add(c10, bg, samples=18, seed=7, sample_mode=H.SAMPLE_RNG)
        for n in ADDS:
            four.add(c10, bg, samples=n, seed=7, sample_mode=H.SAMPLE_RNG)
        want = one.resolve()
        assert want[0].any() and np.array_equal(one.counts(), four.counts()) and np.all(one.counts() == 18)
        same_image(four.resolve(), want, f"{name} {mname}: 3 + 5 + 9 + 1 vs 18")
        if name == "entering-the-mirror-dimension" and mname == "flat":
            monkeypatch.setenv("PORTRAYER_PARK", "0")
            four.reset()
            for n in ADDS:
                four.add(c10, bg, samples=n, seed=7, sample_mode=H.SAMPLE_RNG)
            monkeypatch.delenv("PORTRAYER_PARK")
            same_image(four.resolve(), want, f"{name} {mname}: frames in HBM")
        one.close(); four.close()
        r.close()


# ---- 3. pixel centres, a background per row
def test_pixel_centres_and_background_rows(oracle, host, H):
    scene, cam, _ = all_examples()["soft-shadows"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = default_background(W, HT)
    assert bg.shape == (HT, 3)
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        for _ in range(2):
            film.add(c10, bg, samples=8, seed=3, sample_mode=H.SAMPLE_CENTRE)
        rgb, linear, _ = r.render(c10, W, HT, bg, samples=16, seed=3, sample_mode=H.SAMPLE_CENTRE)
        same_image(film.resolve(), (rgb, linear), f"soft-shadows {mname}: 8 + 8 centre samples vs 16")
        film.close()
        r.close()


# ---- 4. a count per pixel
def test_every_pixel_equals_the_render_with_its_own_count(oracle, host, H):
    scene, cam, _ = all_examples()["glossy-reflection"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(9).uniform(0.0, 1.0, size=(HT, W, 3))
    rect, pixel = (9, 5, 40, 30), (33, 17, 33, 17)  # no edge of rect on a tile boundary
    want_counts = np.full((HT, W), 3, dtype=np.uint32)
    want_counts[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1] = 9
    want_counts[pixel[1], pixel[0]] = 11
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        empty = r.film(W, HT)
        pre_rgb, pre_lin = np.full((HT, W, 3), 201, dtype=np.uint8), np.full((HT, W, 3), -7.25)
        out = empty.resolve(into=pre_rgb, linear_into=pre_lin)
        assert out[0] is pre_rgb and out[1] is pre_lin and np.all(pre_rgb == 201) and np.all(pre_lin == -7.25), "a film without samples writes nothing"
        assert not empty.counts().any()
        empty.close()
        film = r.film(W, HT)
        film.add(c10, bg, samples=3, seed=7, sample_mode=H.SAMPLE_RNG)
        film.add(c10, bg, samples=6, seed=7, sample_mode=H.SAMPLE_RNG, rect=rect)
        film.add(c10, bg, samples=2, seed=7, sample_mode=H.SAMPLE_RNG, rect=pixel)
        film.add(c10, bg, samples=5, seed=7, sample_mode=H.SAMPLE_RNG, rect=(20, 10, 19, 10))  # an inverted slice adds nothing
        counts = film.counts()
        assert np.array_equal(counts, want_counts) and sorted(np.unique(counts)) == [3, 9, 11]
        got = film.resolve()
        for n in (3, 9, 11):
            rgb, linear, _ = r.render(c10, W, HT, bg, samples=n, seed=7, sample_mode=H.SAMPLE_RNG)
            at = counts == n
            assert at.any()
            same_image((got[0][at][None], got[1][at][None]), (rgb[at][None], linear[at][None]), f"glossy-reflection {mname}: the pixels with {n} samples")
        film.close()
        r.close()


# ---- 5. more samples in one add than one launch takes
@pytest.mark.parametrize("samples", [64, 70])
def test_a_long_add(oracle, host, H, samples):
    scene, cam, _ = all_examples()["primitives-simple"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(samples).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        film.add(c10, bg, samples=samples, seed=7, sample_mode=H.SAMPLE_RNG)
        rgb, linear, _ = r.render(c10, W, HT, bg, samples=samples, seed=7, sample_mode=H.SAMPLE_RNG)
        same_image(film.resolve(), (rgb, linear), f"primitives-simple {mname}: one add of {samples}")
        assert np.all(film.counts() == samples)
        film.close()
        r.close()


# ---- 6. reset; the scene moves between a film's lifetimes
def test_reset_and_a_moved_scene(oracle, host, H):
    from test_gpu_update import moved
    make = all_examples()["glossy-reflection"]
    scene, cam, _ = make()
    scene_b, cam_b = moved(make, oracle)
    hs, c10, c10_b = host_glue.host_scene(scene), host_glue.cam10(cam), host_glue.cam10(cam_b)
    hs_b = host_glue.host_scene(scene_b)
    bg = np.random.default_rng(4).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        for n in (5, 6):
            film.add(c10, bg, samples=n, seed=2, sample_mode=H.SAMPLE_RNG)
        first = film.resolve()
        film.reset()
        assert not film.counts().any()
        for n in (5, 6):
            film.add(c10, bg, samples=n, seed=2, sample_mode=H.SAMPLE_RNG)
        same_image(film.resolve(), first, f"{mname}: the same adds after a reset")
        r.update(hs_b)
        film.reset()
        for n in (5, 6):
            film.add(c10_b, bg, samples=n, seed=2, sample_mode=H.SAMPLE_RNG)
        rgb, linear, _ = r.render(c10_b, W, HT, bg, samples=11, seed=2, sample_mode=H.SAMPLE_RNG)
        got = film.resolve()
        same_image(got, (rgb, linear), f"{mname}: the film of the moved scene vs its render")
        assert not np.array_equal(got[0], first[0])
        film.close()
        r.close()


# ---- 7. the device path
def test_device_buffers_on_a_stream_and_the_passes_beside_it(H):
    """pt_film_add_device / pt_film_resolve_device with the background and the outputs in torch tensors on a stream of torch's, closed by pt_radiance_finish, in a
    process of its own in which torch initialises its GPU side first. While the pass is open a radiance pass, a second add and pt_scene_update are refused and
    the film is unharmed; renders on both slots and a rays pass run beside it and keep their bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, ctypes as C
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch
assert torch.cuda.is_available()
dev = torch.device("cuda:0")
x = torch.ones(1024, device=dev); torch.cuda.synchronize()
import numpy as np
from portrayer_amd import _hip as H
from portrayer_amd import host
from scene_dsl import ASSETS
from test_gpu_update import motion_of
lib = H.lib()
w, h = 203, 117
sc = host.Scene.example("entering-the-mirror-dimension", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
ctx = r.context
cam = host.camera(sc.camera, w, h)
rng = np.random.default_rng(1)
bg = rng.uniform(size=(h, w, 3))
# what the calls give one after the other: the film through the host path, two renders, a rays pass
ref_film = r.film(w, h)
ref_film.add(sc.camera, bg, samples=5, seed=2, sample_mode=H.SAMPLE_RNG)
ref_film.add(sc.camera, bg, samples=12, seed=2, sample_mode=H.SAMPLE_RNG)
ref_rgb, ref_lin = ref_film.resolve()
assert ref_rgb.any()
ref_film.close()
renders = [r.render(sc.camera, w, h, bg, samples=8, seed=10 + k, sample_mode=H.SAMPLE_RNG)[0] for k in (0, 1)]
n = 20_000
o = rng.uniform(-6, 6, size=(n, 3)); d = rng.normal(size=(n, 3))
ref_t = r.rays(o, d, want=("t",))["t"]

d_bg = torch.from_numpy(bg).to(dev)
t_rgb = torch.full((h, w, 3), 9, dtype=torch.uint8, device=dev)
t_lin = torch.full((h, w, 3), 5, dtype=torch.float64, device=dev)
d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
d_t = torch.zeros(n, dtype=torch.float64, device=dev)
d_img = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in (0, 1)]
t_rad = torch.zeros((64, 3), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
film = C.c_void_p()
assert lib.pt_film_create(ctx, w, h, C.byref(film)) == H.OK
vp = lambda t: C.c_void_p(t.data_ptr())
full = H.PtRect(0, 0, w - 1, h - 1)
add = lambda samples: lib.pt_film_add_device(ctx, film, C.byref(cam), vp(d_bg), C.byref(H.PtFilmParams(full, samples, 2, H.SAMPLE_RNG, 0)), C.c_void_p(stream.cuda_stream))
assert add(5) == H.OK, lib.pt_last_error(ctx)
# refused while the pass is open, each with PT_ERR_ARGUMENT
assert add(12) == H.ERR_ARGUMENT
qp = H.PtRadianceParams(64, 0, 0, 0, 0, 0)
assert lib.pt_radiance_device(ctx, C.byref(qp), vp(d_o), vp(d_d), vp(d_bg), vp(t_rad), None) == H.ERR_ARGUMENT
keep = []
assert lib.pt_scene_update(ctx, C.byref(motion_of(H, sc, "flat", keep)), None) == H.ERR_ARGUMENT and b"in flight" in lib.pt_last_error(ctx)
counts = np.zeros((h, w), dtype=np.uint32)
assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.ERR_ARGUMENT  # the host reads no film a pass is writing
assert lib.pt_film_reset(ctx, film) == H.ERR_ARGUMENT and lib.pt_film_destroy(ctx, film) == H.ERR_ARGUMENT
# renders on both slots and a rays pass beside it
for k in (0, 1):
    p = H.PtRenderParams(w, h, full, 8, 10 + k, H.SAMPLE_RNG, 0, 0, 1, 0)
    assert lib.pt_render_device(ctx, C.byref(cam), vp(d_bg), C.byref(p), 0, vp(d_img[k]), C.c_void_p(lib.pt_context_stream(ctx, k))) == H.OK, lib.pt_last_error(ctx)
rp = H.PtRaysParams(n, 0, 0)
rb = H.PtRaysBuffers(t=C.cast(vp(d_t), H._dp))
assert lib.pt_rays_device(ctx, C.byref(rp), vp(d_o), vp(d_d), C.byref(rb), None) == H.OK, lib.pt_last_error(ctx)
ms = C.c_double(-1.0)
assert lib.pt_radiance_finish(ctx, C.byref(ms)) == H.OK and ms.value > 0.0
assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight any more
assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.OK and np.all(counts == 5), "the refused calls left the film alone"
assert add(12) == H.OK, lib.pt_last_error(ctx)
assert lib.pt_film_resolve_device(ctx, film, vp(t_rgb), vp(t_lin), C.c_void_p(stream.cuda_stream)) == H.OK  # behind the add on its stream
assert lib.pt_radiance_finish(ctx, None) == H.OK
st = H.PtStats()
assert lib.pt_render_finish(ctx, C.byref(st)) == H.OK and lib.pt_render_finish(ctx, C.byref(st)) == H.OK and lib.pt_rays_finish(ctx, None) == H.OK
stream.synchronize()
torch.cuda.synchronize()
assert t_rgb.cpu().numpy().tobytes() == ref_rgb.tobytes() and t_lin.cpu().numpy().tobytes() == ref_lin.tobytes()
for k in (0, 1):
    assert d_img[k].cpu().numpy().tobytes() == renders[k].tobytes(), k
assert d_t.cpu().numpy().tobytes() == ref_t.tobytes()
assert lib.pt_film_destroy(ctx, film) == H.OK and lib.pt_film_destroy(ctx, film) == H.ERR_ARGUMENT
r.close()
assert (x * 2).sum().item() == 2048.0
print("film into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "film into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the argument errors with a live context
def test_argument_errors(host, H):
    lib = H.lib()
    scene, cam, _ = all_examples()["primitives-simple"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    ctx = r.context
    pc = host.camera(c10, W, HT)
    bg = np.zeros((HT, W, 3))
    dp = lambda a: a.ctypes.data_as(H._dp)
    film = C.c_void_p()
    assert lib.pt_film_create(ctx, 0, HT, C.byref(film)) == H.ERR_ARGUMENT and lib.pt_film_create(ctx, W, 0, C.byref(film)) == H.ERR_ARGUMENT
    assert lib.pt_film_create(ctx, 1 << 16, 1 << 15, C.byref(film)) == H.ERR_ARGUMENT and not film.value  # 2^31 pixels
    assert lib.pt_film_create(ctx, W, HT, None) == H.ERR_ARGUMENT
    assert lib.pt_film_create(ctx, W, HT, C.byref(film)) == H.OK and film.value
    full = (0, 0, W - 1, HT - 1)
    params = lambda rect=full, samples=1, mode=H.SAMPLE_RNG, rows=0: H.PtFilmParams(H.PtRect(*rect), samples, 0, mode, rows)
    add = lambda p, f=film, c=ctx: lib.pt_film_add(c, f, C.byref(pc), dp(bg), C.byref(p), None)
    for p in (params(samples=0), params(mode=2), params(mode=-1), params(rows=2), params(rows=-1)):
        assert add(p) == H.ERR_ARGUMENT
    for rect in ((W, 0, W, 0), (0, HT, 0, HT), (0, 0, W, 0), (0, 0, 0, HT)):
        assert add(params(rect=rect)) == H.ERR_SLICE, rect
    assert lib.pt_film_add(ctx, film, None, dp(bg), C.byref(params()), None) == H.ERR_ARGUMENT
    assert lib.pt_film_add(ctx, film, C.byref(pc), None, C.byref(params()), None) == H.ERR_ARGUMENT
    assert lib.pt_film_add(ctx, film, C.byref(pc), dp(bg), None, None) == H.ERR_ARGUMENT
    assert lib.pt_film_add(ctx, None, C.byref(pc), dp(bg), C.byref(params()), None) == H.ERR_ARGUMENT
    assert lib.pt_film_resolve(ctx, film, None, None) == H.ERR_ARGUMENT
    bare = H.Context()
    other = C.c_void_p()
    assert lib.pt_film_create(bare.handle, W, HT, C.byref(other)) == H.OK  # a film needs no scene ...
    assert add(params(), f=other, c=bare.handle) == H.ERR_NO_SCENE               # ... except to add
    assert add(params(samples=0), f=other, c=bare.handle) == H.ERR_ARGUMENT      # the argument comes first
    counts = np.ones((HT, W), dtype=np.uint32)
    assert lib.pt_film_counts(bare.handle, other, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.OK and not counts.any()
    assert lib.pt_film_reset(bare.handle, other) == H.OK
    for c, f in ((ctx, other), (bare.handle, film)):  # a film of another context
        assert add(params(), f=f, c=c) == H.ERR_ARGUMENT and lib.pt_film_reset(c, f) == H.ERR_ARGUMENT and lib.pt_film_destroy(c, f) == H.ERR_ARGUMENT
        assert lib.pt_film_counts(c, f, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.ERR_ARGUMENT
    bare.close()  # the film dies with its context
    assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.OK and not counts.any(), "every refusal left the film unchanged"
    assert add(params(rect=(3, 3, 2, 3), samples=4)) == H.OK  # an inverted slice adds nothing
    assert add(params(rect=(3, 3, 3, 3), samples=1)) == H.OK
    assert add(params(rect=(3, 3, 3, 3), samples=1 << 31)) == H.ERR_ARGUMENT and b"2^31" in lib.pt_last_error(ctx)  # 1 + 2^31
    assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(C.POINTER(C.c_uint32))) == H.OK and counts.sum() == 1 and counts[3, 3] == 1
    assert lib.pt_film_destroy(ctx, film) == H.OK
    with pytest.raises(ValueError, match="background"):
        r.film(W, HT).add(c10, np.zeros((HT, W)))
    with pytest.raises(ValueError, match="width"):
        r.film(0, HT)
    r.close()
