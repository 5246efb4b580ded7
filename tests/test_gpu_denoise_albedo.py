"""The demodulated denoise on the device (pt_film_denoise_albedo, pt_film_denoise_albedo_device / Film.denoise(albedo=...)): the seed and finish
kernels of pt_denoise_albedo.hip around the unchanged level kernels, against the host replay of the same contract (pt_test_denoise_albedo_host) fed with what
the film and the renderer report: resolve's linear, error() squared with the count-1 rule, counts() and Renderer.guides' buffers.

Every comparison in this file is exact (bits of f64, equality of u8) except the one sanity condition at the end. 67 x 37 films unless said, PT_SAMPLE_RNG."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scene_dsl import ASSETS, default_background  # noqa: E402
from test_denoise_albedo_host import host_denoise_albedo  # noqa: E402
from test_denoise_host import bits  # noqa: E402
from test_gpu_denoise import check_against_the_replay, finished_rgb  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37  # a multiple of 16 (the level kernel's tile) in neither direction
RECT = (9, 5, 40, 30)  # no edge on a tile boundary
SEED = 7


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """The golden assets plus a stand-in for earth_cube.png, which texture-mapping opens and the reference repository lacks (tests/test_examples_extra.py)."""
    from PIL import Image
    d = tmp_path_factory.mktemp("assets")
    for f in os.listdir(ASSETS):
        os.symlink(os.path.join(ASSETS, f), os.path.join(d, f))
    Image.fromarray(np.random.default_rng(3).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)).save(os.path.join(d, "earth_cube.png"))
    return str(d)


def renderer(host, H, assets, name, traverse="FLAT"):
    sc = host.Scene.example(name, assets=assets)
    return host.Renderer(sc, getattr(H, "TRAVERSE_" + traverse), kd_depth=8), sc.camera


def level_zero(film, r, c10):
    """What the filter starts from, as the film and the renderer report it: (linear, variance, counts, node, normal, position, albedo)."""
    w, h = film.width, film.height
    _, lin = film.resolve()
    counts = film.counts()
    with np.errstate(all="ignore"):
        err = film.error()
        my = (lin[..., 0] + lin[..., 1]) + lin[..., 2]
        var = np.where(counts >= 2, err * err, np.where(counts == 1, my * my, 0.0))
    g = r.guides(c10, w, h)
    return lin, var, counts, g["node"], g["normal"], g["position"], g["albedo"]


def check_against_the_albedo_replay(H, film, r, c10, what, iterations, sigma_color=2.0, sigma_plane=0.0, normal_power=32, same_node=False):
    """Film.denoise(albedo=True) into pre-filled buffers == pt_test_denoise_albedo_host over level_zero(), in linear, variance and rgb."""
    w, h = film.width, film.height
    zero = level_zero(film, r, c10)
    npl2 = -1 if normal_power is None else normal_power.bit_length() - 1
    pre = np.full((h, w, 3), 201, dtype=np.uint8), np.full((h, w, 3), -7.25), np.full((h, w), -7.25)
    rgb, lin, var = film.denoise(c10, iterations=iterations, sigma_color=sigma_color, sigma_plane=sigma_plane, normal_power=normal_power, same_node=same_node,
                                 into=pre[0], linear_into=pre[1], variance_into=pre[2], albedo=True)
    want_lin, want_var = host_denoise_albedo(H, *zero, iterations, sigma_color, sigma_plane, npl2, same_node, fill=-7.25)
    for name, got, want in (("linear", lin, want_lin), ("variance", var, want_var)):
        a, b = bits(got), bits(want)
        assert np.array_equal(a, b), "%s, %d levels: %s differs from the host replay in %d of %d values" % (what, iterations, name, int((a != b).sum()), a.size)
    assert np.array_equal(rgb, finished_rgb(H, want_lin, zero[2], 201)), "%s, %d levels: rgb is not resolve's finishing of linear" % (what, iterations)
    return zero, (rgb, lin, var)


# ---- 1. the kernels are the contract
@pytest.mark.parametrize("name,traverse", [("texture-mapping", "FLAT"), ("transmission-refraction", "FLAT"), ("macho-cows", "HIER")])
def test_one_three_and_five_levels_equal_the_host_replay(host, H, assets, name, traverse):
    r, c10 = renderer(host, H, assets, name, traverse)
    film = r.film(W, HT, moments=True)
    film.add(c10, default_background(W, HT), samples=8, seed=SEED, sample_mode=H.SAMPLE_RNG)
    for iterations in (1, 3, 5):
        zero, got = check_against_the_albedo_replay(H, film, r, c10, name, iterations)
        assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert (zero[3] >= 0).any() and zero[1].any() and zero[6].any(), "the scene must hit something, be noisy somewhere and have an albedo"
    _, plain = film.denoise(c10, iterations=3)
    assert bits(plain).tobytes() != bits(got[1]).tobytes() or name == "macho-cows", "on a textured scene the demodulated filter is another filter"
    check_against_the_albedo_replay(H, film, r, c10, name + " plane + same node", 3, sigma_color=1.5, sigma_plane=0.05, normal_power=128, same_node=True)
    check_against_the_albedo_replay(H, film, r, c10, name + " no weight", 2, sigma_color=0.0, sigma_plane=0.0, normal_power=None)
    film.close()
    r.close()


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (17, 33)], ids=lambda s: "%dx%d" % s)
def test_small_films_at_five_levels(host, H, assets, size):
    w, h = size
    r, c10 = renderer(host, H, assets, "normal-mapping")
    film = r.film(w, h, moments=True)
    film.add(c10, default_background(w, h), samples=8, seed=SEED, sample_mode=H.SAMPLE_RNG)
    check_against_the_albedo_replay(H, film, r, c10, "%dx%d" % size, 5)
    check_against_the_albedo_replay(H, film, r, c10, "%dx%d plane" % size, 5, sigma_plane=0.05)
    film.close()
    r.close()


def test_after_a_map_pixels_without_samples_keep_the_buffers_and_feed_no_neighbour(host, H, assets):
    """A map over {0, 1, 3, 8} on a rectangle off the tile grid: counts of 0 (everywhere outside it too), 1 (the count-1 rule), 3 and 8."""
    r, c10 = renderer(host, H, assets, "texture-mapping")
    film = r.film(W, HT, moments=True)
    budget = np.array([0, 1, 3, 8], dtype=np.uint32)[np.random.default_rng(3).integers(0, 4, size=(HT, W))]
    film.add_map(c10, default_background(W, HT), budget, seed=SEED, sample_mode=H.SAMPLE_RNG, rect=RECT)
    counts = film.counts()
    assert sorted(int(v) for v in np.unique(counts)) == [0, 1, 3, 8]
    for iterations in (1, 5):
        zero, (rgb, lin, var) = check_against_the_albedo_replay(H, film, r, c10, "after a map", iterations)
        untouched = counts == 0
        assert np.all(rgb[untouched] == 201) and np.all(lin[untouched] == -7.25) and np.all(var[untouched] == -7.25), "pixels without samples keep the caller's bytes"
        assert np.isfinite(lin[~untouched]).all() and np.isfinite(var[~untouched]).all()
    film.close()
    r.close()


# ---- 2. the two forms of the level kernel
def test_the_direct_and_the_tiled_form_give_identical_bits(host, H, assets, monkeypatch):
    r, c10 = renderer(host, H, assets, "texture-mapping")
    film = r.film(W, HT, moments=True)
    budget = np.array([0, 1, 8, 8], dtype=np.uint32)[np.random.default_rng(5).integers(0, 4, size=(HT, W))]
    film.add_map(c10, default_background(W, HT), budget, seed=SEED, sample_mode=H.SAMPLE_RNG)
    for iterations in (1, 3, 5, 8):
        got = {}
        for tile in ("0", "1"):
            monkeypatch.setenv("PORTRAYER_DENOISE_TILE", tile)
            got[tile] = film.denoise(c10, iterations=iterations, sigma_color=2.0, sigma_plane=0.05, normal_power=32, want_variance=True, albedo=True)
        assert np.array_equal(got["0"][0], got["1"][0]), "%d levels: rgb" % iterations
        assert np.array_equal(bits(got["0"][1]), bits(got["1"][1])) and np.array_equal(bits(got["0"][2]), bits(got["1"][2])), "%d levels: linear / variance" % iterations
    for tile in ("0", "1"):  # ... and each is the contract
        monkeypatch.setenv("PORTRAYER_DENOISE_TILE", tile)
        check_against_the_albedo_replay(H, film, r, c10, "tile=%s" % tile, 5, sigma_plane=0.05)
    film.close()
    r.close()


# ---- 3. the caller's inputs, and what the call leaves alone
def test_the_callers_guides_and_albedo_and_the_film_afterwards(host, H, assets):
    r, c10 = renderer(host, H, assets, "texture-mapping")
    film = r.film(W, HT, moments=True)
    film.add(c10, default_background(W, HT), samples=8, seed=SEED, sample_mode=H.SAMPLE_RNG)
    res_rgb, res_lin = film.resolve()
    on_device = film.denoise(c10, iterations=5, sigma_plane=0.05, want_variance=True, albedo=True)
    g = r.guides(c10, W, HT)
    by_arrays = film.denoise(None, iterations=5, sigma_plane=0.05, want_variance=True, guides=g, albedo=g["albedo"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(on_device, by_arrays)), "the caller's guides and albedo == the guides pass's"
    other = film.denoise(None, iterations=5, sigma_plane=0.05, want_variance=True, guides=g, albedo=np.full((HT, W, 3), 1.0 - H.DENOISE_ALBEDO_EPS))
    plain = film.denoise(c10, iterations=5, sigma_plane=0.05, want_variance=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(other, plain)), "an albedo of 1 - EPS is the plain filter"
    assert on_device[1].tobytes() != plain[1].tobytes()
    # the library's own refusals: the caller's guides without the caller's albedo and the reverse, nothing written
    lin = np.full((HT, W, 3), -7.25)
    p = H.PtDenoiseParams(5, 0, 2.0, 0.0, 5)
    hg = H.PtDenoiseGuides(g["position"].ctypes.data, g["normal"].ctypes.data, g["node"].ctypes.data)
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert host.lib().ph_renderer_film_denoise_albedo(r._h, film._h, dp(c10), C.byref(p), C.byref(hg), None, None, dp(lin), None) < 0 and b"albedo" in host.lib().ph_last_error()
    assert host.lib().ph_renderer_film_denoise_albedo(r._h, film._h, dp(c10), C.byref(p), None, dp(g["albedo"]), None, dp(lin), None) < 0
    assert np.all(lin == -7.25)
    # the film is not written: resolve is what it was, and denoise() without albedo is still its own replay
    again = film.resolve()
    assert again[0].tobytes() == res_rgb.tobytes() and again[1].tobytes() == res_lin.tobytes()
    check_against_the_replay(H, film, r, c10, "without albedo, afterwards", 5)
    film.close()
    r.close()


def test_the_device_path_on_a_stream(H, assets):
    """pt_film_denoise_albedo_device with the guides, the albedo and the outputs in torch tensors on a stream of torch's, in a process of its own in which torch
    initialises its GPU side first: the bits of the host path; refused for a NULL albedo and for an albedo that is not (aligned) device memory."""
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
lib = H.lib()
w, h = 67, 37
sc = host.Scene.example("texture-mapping", assets=%r)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
ctx = r.context
cam = host.camera(sc.camera, w, h)
bg = np.random.default_rng(1).uniform(size=(h, w, 3))
g = r.guides(sc.camera, w, h)
ref = r.film(w, h, moments=True)
ref.add(sc.camera, bg, samples=8, seed=2, sample_mode=H.SAMPLE_RNG)
ref_rgb, ref_lin, ref_var = ref.denoise(sc.camera, iterations=5, sigma_color=2.0, sigma_plane=0.05, normal_power=32, want_variance=True, albedo=True)
plain = ref.denoise(sc.camera, iterations=5, sigma_color=2.0, sigma_plane=0.05, normal_power=32, want_variance=True)
assert ref_rgb.any() and ref_lin.tobytes() != plain[1].tobytes()
ref.close()

t_pos, t_nrm, t_node, t_alb = (torch.from_numpy(g[k]).to(dev) for k in ("position", "normal", "node", "albedo"))
t_rgb = torch.full((h, w, 3), 9, dtype=torch.uint8, device=dev)
t_lin = torch.full((h, w, 3), 5, dtype=torch.float64, device=dev)
t_var = torch.full((h, w), 5, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
s = C.c_void_p(stream.cuda_stream)
film = C.c_void_p()
assert lib.pt_film_create_moments(ctx, w, h, C.byref(film)) == H.OK
vp = lambda t: C.c_void_p(t.data_ptr())
fp = H.PtFilmParams(H.PtRect(0, 0, w - 1, h - 1), 8, 2, H.SAMPLE_RNG, 0)
assert lib.pt_film_add(ctx, film, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(fp), None) == H.OK, lib.pt_last_error(ctx)
p = H.PtDenoiseParams(5, 0, 2.0, 0.05, 5)
gd = H.PtDenoiseGuides(t_pos.data_ptr(), t_nrm.data_ptr(), t_node.data_ptr())
denoise = lambda alb: lib.pt_film_denoise_albedo_device(ctx, film, C.byref(p), C.byref(gd), alb, vp(t_rgb), vp(t_lin), vp(t_var), s)
# (Pinned host memory and an interior pointer of a tensor: neither could fault even if the check were wrong; a buffer that is too short is deliberately not tried.)
pin_alb = torch.from_numpy(g["albedo"]).pin_memory()
assert denoise(None) == H.ERR_ARGUMENT and b"albedo" in lib.pt_last_error(ctx)
assert denoise(vp(pin_alb)) == H.ERR_ARGUMENT and b"not device memory" in lib.pt_last_error(ctx)
assert denoise(C.c_void_p(t_alb.data_ptr() + 4)) == H.ERR_ARGUMENT and b"aligned" in lib.pt_last_error(ctx)
assert lib.pt_film_denoise_albedo_device(ctx, film, C.byref(H.PtDenoiseParams(5, 2, 2.0, 0.05, 5)), C.byref(gd), vp(t_alb), vp(t_rgb), vp(t_lin), vp(t_var), s) == H.ERR_ARGUMENT
stream.synchronize()
assert (t_rgb.cpu().numpy() == 9).all() and (t_lin.cpu().numpy() == 5).all() and (t_var.cpu().numpy() == 5).all(), "a refused call writes nothing"
assert denoise(vp(t_alb)) == H.OK, lib.pt_last_error(ctx)
stream.synchronize()
assert t_rgb.cpu().numpy().tobytes() == ref_rgb.tobytes() and t_lin.cpu().numpy().tobytes() == ref_lin.tobytes() and t_var.cpu().numpy().tobytes() == ref_var.tobytes()
# the host-buffer form of the library
hg = H.PtDenoiseGuides(g["position"].ctypes.data, g["normal"].ctypes.data, g["node"].ctypes.data)
out = np.full((h, w, 3), 7.0)
assert lib.pt_film_denoise_albedo(ctx, film, C.byref(p), C.byref(hg), None, None, out.ctypes.data_as(H._dp), None) == H.ERR_ARGUMENT and (out == 7.0).all()
assert lib.pt_film_denoise_albedo(ctx, film, C.byref(p), C.byref(hg), g["albedo"].ctypes.data_as(H._dp), None, out.ctypes.data_as(H._dp), None) == H.OK, lib.pt_last_error(ctx)
assert out.tobytes() == ref_lin.tobytes()
assert lib.pt_film_destroy(ctx, film) == H.OK
r.close()
assert (x * 2).sum().item() == 2048.0
print("a demodulated device denoise into torch tensors ok")
""" % (root, root, assets)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "a demodulated device denoise into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
