"""The film's lens on the device (pt_film_add_lens / Film.add(lens=)): with no aperture a thin lens IS the pinhole, so a lens film equals a plain
film in every bit; with a real lens every sample equals what Renderer.radiance answers for the contract's ray (pt_test_lens_rays_host) with the pixel's stream,
the sample's index and the pixel's background, folded as the film folds (pt_test_film_fold_host) and divided as resolve divides - in all three traversals.

Every comparison in this file is exact: bits() equality of f64 and equality of u8 and u32. No case is left out of a comparison."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from lens_restate import replay  # noqa: E402
from test_gpu_aov import bits, modes  # noqa: E402
from test_gpu_radiance import all_examples  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 19, 11  # 3 x 2 tiles of 8 x 8, partial on both edges
ADDS = (5, 6)   # crosses the 8-sample chunk; 5 and 6 samples leave idle lanes at K = 8
SEED = 7
RECT = (3, 2, 14, 8)  # no corner on a tile border


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def load(name):
    """(the host library's scene, its 10 camera numbers): a scene of tests/example_scenes.py as tests/test_gpu_film.py loads it, else the library's own example"""
    if name in all_examples():
        scene, cam, _ = all_examples()[name]()
        return host_glue.host_scene(scene), host_glue.cam10(cam)
    from portrayer_amd import host
    from scene_dsl import ASSETS
    sc = host.Scene.example(name, assets=ASSETS)
    return sc, np.asarray(sc.camera, dtype=np.float64)


def lenses(host, c10):
    """One real lens per model for the camera c10: focused on the point the camera looks at, the orthographic window framed like the perspective view there."""
    focus = float(np.linalg.norm(c10[3:6] - c10[0:3]))
    return {"thin": host.Lens.thin(0.04 * focus, focus), "ortho": host.Lens.ortho(focus * float(np.tan(c10[9] / 2.0))), "fisheye": host.Lens.fisheye(150.0)}


def background(w, h, tag):
    return np.random.default_rng(tag).uniform(0.0, 1.0, size=(h, w, 3))


def same_film(a, b, what):
    assert np.array_equal(a.counts(), b.counts()), what + ": counts"
    (rgb_a, lin_a), (rgb_b, lin_b) = a.resolve(), b.resolve()
    assert np.array_equal(bits(lin_a), bits(lin_b)), "%s: linear differs in %d values" % (what, int((bits(lin_a) != bits(lin_b)).sum()))
    assert np.array_equal(rgb_a, rgb_b), what + ": rgb"
    return rgb_a


# ---- 1. no aperture: the pinhole
@pytest.mark.parametrize("name", ["soft-shadows", "glossy-reflection", "transmission-refraction", "simple-cows"])
def test_a_thin_lens_without_an_aperture_is_film_add_bit_for_bit(oracle, host, H, name):
    hs, c10 = load(name)
    bg = background(W, HT, 1)
    pinhole = host.Lens.thin(0.0, 3.0)
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        plain, lens, mixed = r.film(W, HT), r.film(W, HT), r.film(W, HT)
        for i, n in enumerate(ADDS):
            plain.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG)
            lens.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=pinhole)
            mixed.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=pinhole if i == 0 else None)
            rgb = same_film(lens, plain, "%s %s after %d" % (name, mname, n))
            same_film(mixed, plain, "%s %s after %d, lens and plain adds interleaved" % (name, mname, n))
        assert rgb.any() and np.all(plain.counts() == sum(ADDS))
        mixed.add(c10, bg, samples=3, seed=SEED, sample_mode=H.SAMPLE_CENTRE, lens=pinhole, rect=RECT)
        plain.add(c10, bg, samples=3, seed=SEED, sample_mode=H.SAMPLE_CENTRE, rect=RECT)
        same_film(mixed, plain, "%s %s: pixel centres over a slice" % (name, mname))
        for f in (plain, lens, mixed):
            f.close()
        r.close()


# ---- 2. a real lens: the chain of the header's promise
_CHAIN = {}


def chain(H, host, r, key, c10, lens, w, h, bg, cuts, sample_mode):
    """Per pixel the samples the promise names and their sum: pt_test_lens_rays_host's rays of the whole image in pixel order, Renderer.radiance per sample index
    with stream_base = 0, sample = s and the background per ray, pt_test_film_fold_host over the adds `cuts`. -> samples (n, h * w, 3), sum (h * w, 3).
    Computed once per key and left unchanged."""
    if key in _CHAIN:
        return _CHAIN[key]
    pc = host.camera(c10, w, h)
    xy = np.array([(x, y) for y in range(h) for x in range(w)], dtype=np.uint32)
    l = lens.struct()
    n = sum(cuts)
    samples = np.zeros((n, h * w, 3))
    for s in range(n):
        O, D = replay(H, pc, (l.model, l.aperture, l.focus, l.extent), w, h, SEED, sample_mode, xy, np.full(len(xy), s, dtype=np.uint32))
        samples[s] = r.radiance(O, D, background=bg.reshape(-1, 3), seed=SEED, sample=s, stream_base=0)["rgb"]
    total = np.zeros((h * w, 3))
    cu = (C.c_uint32 * len(cuts))(*cuts)
    for p in range(h * w):
        one = np.ascontiguousarray(samples[:, p, :])
        assert H.lib().pt_test_film_fold_host(n, one.ctypes.data_as(H._dp), cu, len(cuts), total[p].ctypes.data_as(H._dp)) == H.OK
    samples.setflags(write=False); total.setflags(write=False)
    _CHAIN[key] = (samples, total)
    return _CHAIN[key]


@pytest.mark.parametrize("sample_mode", [0, 1], ids=["centre", "rng"])
@pytest.mark.parametrize("model", ["thin", "ortho", "fisheye"])
def test_every_sample_is_radiance_along_the_contracts_ray(oracle, host, H, model, sample_mode):
    name = "glossy-reflection"  # draws behind the primary ray: the glossy material and the area light
    hs, c10 = load(name)
    lens = lenses(host, c10)[model]
    bg = background(W, HT, 2)
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        _, total = chain(H, host, r, (name, mname, model, sample_mode), c10, lens, W, HT, bg, ADDS, sample_mode)
        film = r.film(W, HT)
        for n in ADDS:
            film.add(c10, bg, samples=n, seed=SEED, sample_mode=sample_mode, lens=lens)
        assert np.all(film.counts() == sum(ADDS))
        rgb, linear = film.resolve()
        want = total / float(sum(ADDS))
        assert np.array_equal(bits(linear.reshape(-1, 3)), bits(want)), "%s %s %s: %d values differ" % (name, mname, model, int((bits(linear.reshape(-1, 3)) != bits(want)).sum()))
        plain = r.film(W, HT)
        plain.add(c10, bg, samples=sum(ADDS), seed=SEED, sample_mode=sample_mode)
        pinhole_rgb = plain.resolve()[0]
        assert not np.array_equal(rgb, pinhole_rgb), "a real lens is no pinhole"
        hit = (bits(linear) != bits(np.broadcast_to(bg, linear.shape))).any(axis=2)
        assert hit.any(), "the lens sees the scene"
        # a slice with both corners off tile borders: the same samples inside, nothing outside
        part = r.film(W, HT)
        for n in ADDS:
            part.add(c10, bg, samples=n, seed=SEED, sample_mode=sample_mode, lens=lens, rect=RECT)
        inside = np.zeros((HT, W), dtype=bool)
        inside[RECT[1]:RECT[3] + 1, RECT[0]:RECT[2] + 1] = True
        assert np.array_equal(part.counts(), np.where(inside, sum(ADDS), 0).astype(np.uint32))
        pre_rgb, pre_lin = np.full((HT, W, 3), 201, dtype=np.uint8), np.full((HT, W, 3), -7.25)
        part.resolve(into=pre_rgb, linear_into=pre_lin)
        assert np.array_equal(bits(pre_lin[inside]), bits(linear[inside])) and np.array_equal(pre_rgb[inside], rgb[inside])
        assert np.all(pre_lin[~inside] == -7.25) and np.all(pre_rgb[~inside] == 201), "pixels outside the slice are untouched"
        for f in (film, plain, part):
            f.close()
        r.close()


def test_a_long_add_crosses_the_rotation_round_and_takes_several_launches(oracle, host, H):
    """60 + 8 on a 9 x 5 film: samples 60 .. 67 of the second add straddle s = 64, where the lens points' round and rotation change, and each add is several
    launches of at most PT_FILM_LW samples."""
    w, h, cuts = 9, 5, (60, 8)
    name = "soft-shadows"
    hs, c10 = load(name)
    lens = lenses(host, c10)["thin"]
    bg = background(w, h, 3)
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        _, total = chain(H, host, r, (name, mname, "long"), c10, lens, w, h, bg, cuts, H.SAMPLE_RNG)
        film = r.film(w, h)
        for n in cuts:
            film.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=lens)
        assert np.all(film.counts() == sum(cuts))
        linear = film.resolve()[1]
        want = total / float(sum(cuts))
        assert np.array_equal(bits(linear.reshape(-1, 3)), bits(want)), "%s %s: %d values differ" % (name, mname, int((bits(linear.reshape(-1, 3)) != bits(want)).sum()))
        film.close()
        r.close()


# ---- 3. a film with moments
def test_the_error_of_a_moments_film_behind_a_lens(oracle, host, H):
    name = "glossy-reflection"
    hs, c10 = load(name)
    bg = background(W, HT, 2)
    lens = lenses(host, c10)["thin"]
    pinhole = host.Lens.thin(0.0, 1.0)
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        plain, zero, real = r.film(W, HT, moments=True), r.film(W, HT, moments=True), r.film(W, HT, moments=True)
        for n in ADDS:
            plain.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG)
            zero.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=pinhole)
            real.add(c10, bg, samples=n, seed=SEED, sample_mode=H.SAMPLE_RNG, lens=lens)
        assert np.array_equal(bits(zero.error()), bits(plain.error())), mname
        same_film(zero, plain, "%s %s moments" % (name, mname))
        samples, total = chain(H, host, r, (name, mname, "thin", H.SAMPLE_RNG), c10, lens, W, HT, bg, ADDS, H.SAMPLE_RNG)
        want = np.zeros(HT * W)
        cu = (C.c_uint32 * len(ADDS))(*ADDS)
        out, q, e = np.zeros(3), C.c_double(0.0), C.c_double(0.0)
        for p in range(HT * W):
            one = np.ascontiguousarray(samples[:, p, :])
            assert H.lib().pt_test_film_moments_host(len(one), one.ctypes.data_as(H._dp), cu, len(ADDS), out.ctypes.data_as(H._dp), C.byref(q), C.byref(e)) == H.OK
            assert np.array_equal(bits(out), bits(total[p]))
            want[p] = e.value
        err = real.error()
        assert np.array_equal(bits(err.ravel()), bits(want)), "%s: %d errors differ" % (mname, int((bits(err.ravel()) != bits(want)).sum()))
        assert np.isfinite(err).all() and (err > 0.0).any()
        for f in (plain, zero, real):
            f.close()
        r.close()


# ---- 4. the device path
def test_device_buffers_on_a_stream_behind_other_passes(H):
    """pt_film_add_lens_device with the background in a torch tensor on a stream of torch's, behind a rays pass queued on that stream and beside a render, closed by
    pt_radiance_finish, in a process of its own in which torch initialises its GPU side first. While the pass is open a second add of either kind and a radiance
    pass are refused and the film is unharmed. The argument errors of a live context come through the library with their own words and leave the film alone."""
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
lib = H.lib()
w, h = 19, 11
sc = host.Scene.example("glossy-reflection", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_KD, kd_depth=8)
ctx = r.context
cam = host.camera(sc.camera, w, h)
rng = np.random.default_rng(1)
bg = rng.uniform(size=(h, w, 3))
lens = host.Lens.thin(0.3, 6.0)
ls = lens.struct()
ref_film = r.film(w, h)
for n in (5, 6):
    ref_film.add(sc.camera, bg, samples=n, seed=2, sample_mode=H.SAMPLE_RNG, lens=lens)
ref_rgb, ref_lin = ref_film.resolve()
assert ref_rgb.any()
ref_film.close()
ref_img = r.render(sc.camera, w, h, bg, samples=4, seed=10, sample_mode=H.SAMPLE_RNG)[0]
n = 4096
o = rng.uniform(-6, 6, size=(n, 3)); d = rng.normal(size=(n, 3))
ref_t = r.rays(o, d, want=("t",))["t"]

d_bg = torch.from_numpy(bg).to(dev)
t_rgb = torch.full((h, w, 3), 9, dtype=torch.uint8, device=dev)
t_lin = torch.full((h, w, 3), 5, dtype=torch.float64, device=dev)
d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
d_t = torch.zeros(n, dtype=torch.float64, device=dev)
d_img = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
t_rad = torch.zeros((64, 3), dtype=torch.float64, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
st_p = C.c_void_p(stream.cuda_stream)
vp = lambda t: C.c_void_p(t.data_ptr())
full = H.PtRect(0, 0, w - 1, h - 1)
film = C.c_void_p()
assert lib.pt_film_create(ctx, w, h, C.byref(film)) == H.OK
counts = np.ones((h, w), dtype=np.uint32)
u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
params = lambda samples=5, mode=H.SAMPLE_RNG, rect=full: H.PtFilmParams(rect, samples, 2, mode, 0)
add = lambda samples, l=ls: lib.pt_film_add_lens_device(ctx, film, C.byref(cam), C.byref(l) if l is not None else None, vp(d_bg), C.byref(params(samples)), st_p)

# the argument errors, live: every one PT_ERR_ARGUMENT with its own words, nothing queued, the film unchanged
nan, inf = float("nan"), float("inf")
for l, word in ((None, b"NULL lens"), (H.PtLens(3, 0.0, 1.0, 1.0), b"unknown lens model"), (H.PtLens(-1, 0.0, 1.0, 1.0), b"unknown lens model"),
                (H.PtLens(H.LENS_THIN, -1.0, 1.0, 1.0), b"aperture"), (H.PtLens(H.LENS_THIN, nan, 1.0, 1.0), b"aperture"), (H.PtLens(H.LENS_THIN, inf, 1.0, 1.0), b"aperture"),
                (H.PtLens(H.LENS_THIN, 0.1, 0.0, 1.0), b"focus"), (H.PtLens(H.LENS_THIN, 0.1, nan, 1.0), b"focus"), (H.PtLens(H.LENS_THIN, 0.1, inf, 1.0), b"focus"),
                (H.PtLens(H.LENS_ORTHO, 0.0, 1.0, 0.0), b"extent"), (H.PtLens(H.LENS_ORTHO, 0.0, 1.0, nan), b"extent"), (H.PtLens(H.LENS_STEREO, 0.0, 1.0, -1.0), b"extent"),
                (H.PtLens(H.LENS_STEREO, 0.0, 1.0, inf), b"extent")):
    assert add(5, l) == H.ERR_ARGUMENT and word in lib.pt_last_error(ctx), (word, lib.pt_last_error(ctx))
    hb = lib.pt_film_add_lens(ctx, film, C.byref(cam), C.byref(l) if l is not None else None, bg.ctypes.data_as(H._dp), C.byref(params()), None)
    assert hb == H.ERR_ARGUMENT and word in lib.pt_last_error(ctx), word
# pt_film_add's own refusals come first
assert lib.pt_film_add_lens_device(ctx, film, C.byref(cam), None, vp(d_bg), C.byref(params(0)), st_p) == H.ERR_ARGUMENT and b"samples" in lib.pt_last_error(ctx)
assert lib.pt_film_add_lens_device(ctx, film, C.byref(cam), None, vp(d_bg), C.byref(params(5, 2)), st_p) == H.ERR_ARGUMENT and b"sample_mode" in lib.pt_last_error(ctx)
assert lib.pt_film_add_lens_device(ctx, film, C.byref(cam), None, vp(d_bg), C.byref(params(5, rect=H.PtRect(0, 0, w, 0))), st_p) == H.ERR_SLICE
assert lib.pt_film_add_lens_device(ctx, film, None, C.byref(ls), vp(d_bg), C.byref(params()), st_p) == H.ERR_ARGUMENT
assert lib.pt_film_add_lens_device(ctx, None, C.byref(cam), C.byref(ls), vp(d_bg), C.byref(params()), st_p) == H.ERR_ARGUMENT
assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT  # nothing was queued
assert lib.pt_film_counts(ctx, film, u32(counts)) == H.OK and not counts.any(), "every refusal left the film unchanged"
assert lib.pt_film_add_lens_device(ctx, film, C.byref(cam), C.byref(ls), vp(d_bg), C.byref(params(5, rect=H.PtRect(3, 3, 2, 3))), st_p) == H.OK  # an inverted slice queues nothing
assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT

# a render and a rays pass on the stream, the lens add behind them
p = H.PtRenderParams(w, h, full, 4, 10, H.SAMPLE_RNG, 0, 0, 1, 0)
assert lib.pt_render_device(ctx, C.byref(cam), vp(d_bg), C.byref(p), 0, vp(d_img), C.c_void_p(lib.pt_context_stream(ctx, 0))) == H.OK, lib.pt_last_error(ctx)
rp = H.PtRaysParams(n, 0, 0)
rb = H.PtRaysBuffers(t=C.cast(vp(d_t), H._dp))
assert lib.pt_rays_device(ctx, C.byref(rp), vp(d_o), vp(d_d), C.byref(rb), st_p) == H.OK, lib.pt_last_error(ctx)
assert add(5) == H.OK, lib.pt_last_error(ctx)
# refused while the pass is open, each with PT_ERR_ARGUMENT
assert add(6) == H.ERR_ARGUMENT and b"in flight" in lib.pt_last_error(ctx)
assert lib.pt_film_add_device(ctx, film, C.byref(cam), vp(d_bg), C.byref(params(6)), st_p) == H.ERR_ARGUMENT
assert lib.pt_film_add_lens(ctx, film, C.byref(cam), C.byref(ls), bg.ctypes.data_as(H._dp), C.byref(params(6)), None) == H.ERR_ARGUMENT
qp = H.PtRadianceParams(64, 0, 0, 0, 0, 0)
assert lib.pt_radiance_device(ctx, C.byref(qp), vp(d_o), vp(d_d), vp(d_bg), vp(t_rad), None) == H.ERR_ARGUMENT
assert lib.pt_film_counts(ctx, film, u32(counts)) == H.ERR_ARGUMENT  # the host reads no film a pass is writing
assert lib.pt_film_reset(ctx, film) == H.ERR_ARGUMENT and lib.pt_film_destroy(ctx, film) == H.ERR_ARGUMENT
ms = C.c_double(-1.0)
assert lib.pt_radiance_finish(ctx, C.byref(ms)) == H.OK and ms.value > 0.0
assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight any more
assert lib.pt_film_counts(ctx, film, u32(counts)) == H.OK and np.all(counts == 5), "the refused calls left the film alone"
assert add(6) == H.OK, lib.pt_last_error(ctx)
assert lib.pt_film_resolve_device(ctx, film, vp(t_rgb), vp(t_lin), st_p) == H.OK  # behind the add on its stream
assert lib.pt_radiance_finish(ctx, None) == H.OK
st = H.PtStats()
assert lib.pt_render_finish(ctx, C.byref(st)) == H.OK and lib.pt_rays_finish(ctx, None) == H.OK
stream.synchronize()
torch.cuda.synchronize()
assert t_rgb.cpu().numpy().tobytes() == ref_rgb.tobytes() and t_lin.cpu().numpy().tobytes() == ref_lin.tobytes()
assert d_img.cpu().numpy().tobytes() == ref_img.tobytes()
assert d_t.cpu().numpy().tobytes() == ref_t.tobytes()
assert lib.pt_film_destroy(ctx, film) == H.OK
r.close()
assert (x * 2).sum().item() == 2048.0
print("lens film into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "lens film into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
