"""The adaptive film (pt_film_add_map, pt_film_error, pt_film_budget_device / Film.add_map, Film.error, Film.refine): a sample budget per pixel, a
noise estimate and the closed loop on the device - and still every pixel carries the bits of a render with that pixel's own count of samples.

Every comparison in this file is exact: bits() equality of f64, equality of u8 and u32. 67 x 37 film, kd_depth=8, all three traversals, as tests/test_gpu_film.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from test_film_plan import BUDGETS, LW, host_plan  # noqa: E402
from test_gpu_aov import bits, modes  # noqa: E402
from test_gpu_film import same_image  # noqa: E402
from test_gpu_radiance import all_examples  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37  # a multiple of 8 in neither direction
RECT = (9, 5, 40, 30)  # no edge on a tile boundary
SECOND = np.array([0, 2, 8], dtype=np.uint32)
PLAN_BLOCK = 256  # PT_FILM_PLAN_BLOCK: slots, and block sums, per block of the plan kernels


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def seeded_maps():
    """The two budget maps of test 1 and the counts they leave. The closed form first: a pixel outside RECT ends with a value of BUDGETS, one inside with a + b,
    a of BUDGETS, b of SECOND - {0, 1, 3, 8, 9, 17} and {0, 1, 2, 3, 5, 8, 9, 10, 11, 16, 17, 19, 25}: 13 values, 12 of them counts a render can be asked for
    (every one at most 25 samples at 67 x 37). The seed is kept only because its maps reach all of them."""
    rng = np.random.default_rng(11)
    first = BUDGETS[rng.integers(0, len(BUDGETS), size=(HT, W))]
    second = SECOND[rng.integers(0, len(SECOND), size=(HT, W))]  # read inside RECT only
    counts = first.copy()
    x0, y0, x1, y1 = RECT
    counts[y0:y1 + 1, x0:x1 + 1] += second[y0:y1 + 1, x0:x1 + 1]
    closed_form = sorted({int(a) for a in BUDGETS} | {int(a) + int(b) for a in BUDGETS for b in SECOND})
    assert closed_form == [0, 1, 2, 3, 5, 8, 9, 10, 11, 16, 17, 19, 25]
    assert sorted(int(v) for v in np.unique(counts)) == closed_form, "the seeded maps must reach every count of the closed form"
    return first, second, counts


def each_count_is_its_render(r, H, c10, bg, got, counts, seed, sample_mode, what):
    """For every distinct count > 0: the film's pixels with that count == the render with that many samples."""
    for n in sorted(int(v) for v in np.unique(counts) if v > 0):
        rgb, linear, _ = r.render(c10, W, HT, bg, samples=n, seed=seed, sample_mode=sample_mode)
        at = counts == n
        same_image((got[0][at][None], got[1][at][None]), (rgb[at][None], linear[at][None]), "%s: the pixels with %d samples" % (what, n))


# ---- 1. a budget per pixel
@pytest.mark.parametrize("name", ["glossy-reflection", "soft-shadows", "entering-the-mirror-dimension", "transmission-refraction"])
def test_every_pixel_equals_the_render_with_the_count_its_budgets_gave_it(oracle, host, H, name):
    """Random draws (glossy material, area light), the chain and dielectrics. Two adds: a map over {0, 1, 3, 8, 9, 17} on the whole film (three launch rounds), a
    map over {0, 2, 8} on a rectangle off the tile grid."""
    scene, cam, _ = all_examples()[name]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(9).uniform(0.0, 1.0, size=(HT, W, 3))
    first, second, want_counts = seeded_maps()
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        film.add_map(c10, bg, first, seed=7, sample_mode=H.SAMPLE_RNG)
        assert np.array_equal(film.counts(), first)
        film.add_map(c10, bg, second, seed=7, sample_mode=H.SAMPLE_RNG, rect=RECT)
        counts = film.counts()
        assert np.array_equal(counts, want_counts)
        pre_rgb, pre_lin = np.full((HT, W, 3), 201, dtype=np.uint8), np.full((HT, W, 3), -7.25)
        got = film.resolve(into=pre_rgb, linear_into=pre_lin)
        each_count_is_its_render(r, H, c10, bg, got, counts, 7, H.SAMPLE_RNG, "%s %s" % (name, mname))
        untouched = counts == 0
        assert untouched.any() and np.all(got[0][untouched] == 201) and np.all(got[1][untouched] == -7.25), "pixels without samples keep the caller's bytes"
        film.close()
        r.close()


# ---- 2. edge cases of the map
def test_zeros_one_pixel_a_uniform_map_and_max_samples(oracle, host, H):
    scene, cam, _ = all_examples()["glossy-reflection"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(2).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT)
        # a map of zeros: nothing changes (also with a budget outside the rectangle, which is not read)
        zeros = np.zeros((HT, W), dtype=np.uint32)
        assert film.add_map(c10, bg, zeros, seed=7, sample_mode=H.SAMPLE_RNG) == 0.0
        outside = zeros.copy()
        outside[0, 0] = 5
        film.add_map(c10, bg, outside, seed=7, sample_mode=H.SAMPLE_RNG, rect=RECT)
        assert not film.counts().any()
        pre = np.full((HT, W, 3), 201, dtype=np.uint8)
        assert np.all(film.resolve(into=pre)[0] == 201)
        # a single pixel with budget 1
        one = zeros.copy()
        one[17, 33] = 1
        film.add_map(c10, bg, one, seed=7, sample_mode=H.SAMPLE_RNG)
        assert np.array_equal(film.counts(), one)
        rgb, linear, _ = r.render(c10, W, HT, bg, samples=1, seed=7, sample_mode=H.SAMPLE_RNG)
        got = film.resolve()
        assert np.array_equal(got[0][17, 33], rgb[17, 33]) and np.array_equal(bits(got[1][17, 33]), bits(linear[17, 33]))
        # a uniform budget of 8 == add(samples=8), state against state (on top of the one pixel's sample: counts of 8 and 9)
        plain = r.film(W, HT)
        plain.add_map(c10, bg, one, seed=7, sample_mode=H.SAMPLE_RNG)
        plain.add(c10, bg, samples=8, seed=7, sample_mode=H.SAMPLE_RNG)
        film.add_map(c10, bg, np.full((HT, W), 8, dtype=np.uint32), seed=7, sample_mode=H.SAMPLE_RNG)
        assert np.array_equal(film.counts(), plain.counts()) and np.array_equal(film.counts(), one + 8)
        same_image(film.resolve(), plain.resolve(), "%s: a uniform map of 8 vs add(8)" % mname)
        # max_samples = 5 against budgets of 17
        film.reset()
        film.add_map(c10, bg, np.full((HT, W), 17, dtype=np.uint32), seed=7, sample_mode=H.SAMPLE_RNG, max_samples=5)
        assert np.all(film.counts() == 5)
        rgb, linear, _ = r.render(c10, W, HT, bg, samples=5, seed=7, sample_mode=H.SAMPLE_RNG)
        same_image(film.resolve(), (rgb, linear), "%s: max_samples 5 vs the render of 5" % mname)
        film.close(); plain.close()
        r.close()


# ---- 3. the device path
def test_a_device_map_on_a_stream(H):
    """pt_film_add_map_device with the map and the background in torch tensors on a stream of torch's, closed by pt_radiance_finish, in a process of its own in
    which torch initialises its GPU side first: the bits of the host path; the refusals while the pass is open; the host's copy of the counts, an upper bound
    until pt_film_counts."""
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
w, h = 67, 37
sc = host.Scene.example("entering-the-mirror-dimension", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
ctx = r.context
cam = host.camera(sc.camera, w, h)
rng = np.random.default_rng(1)
bg = rng.uniform(size=(h, w, 3))
budget = np.array([0, 1, 3, 8, 9, 17], dtype=np.uint32)[rng.integers(0, 6, size=(h, w))]
ref = r.film(w, h, moments=True)
ref.add(sc.camera, bg, samples=3, seed=2, sample_mode=H.SAMPLE_RNG)
ref.add_map(sc.camera, bg, budget, seed=2, sample_mode=H.SAMPLE_RNG, max_samples=12)
ref_rgb, ref_lin = ref.resolve()
ref_err, ref_counts = ref.error(), ref.counts()
assert ref_rgb.any() and np.array_equal(ref_counts, 3 + np.minimum(budget, 12))
ref.close()

d_bg = torch.from_numpy(bg).to(dev)
d_budget = torch.from_numpy(budget.astype(np.int32)).to(dev)  # (the same 32 bits)
t_rgb = torch.full((h, w, 3), 9, dtype=torch.uint8, device=dev)
t_lin = torch.full((h, w, 3), 5, dtype=torch.float64, device=dev)
t_err = torch.full((h, w), 5, dtype=torch.float64, device=dev)
t_out_budget = torch.zeros((h, w), dtype=torch.int32, device=dev)
t_summary = torch.zeros(2, dtype=torch.int64, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
s = C.c_void_p(stream.cuda_stream)
film = C.c_void_p()
assert lib.pt_film_create_moments(ctx, w, h, C.byref(film)) == H.OK
vp = lambda t: C.c_void_p(t.data_ptr())
full = H.PtRect(0, 0, w - 1, h - 1)
up = C.POINTER(C.c_uint32)
counts = np.zeros((h, w), dtype=np.uint32)
add = lambda samples: lib.pt_film_add(ctx, film, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(H.PtFilmParams(full, samples, 2, H.SAMPLE_RNG, 0)), None)
add_map = lambda mx: lib.pt_film_add_map_device(ctx, film, C.byref(cam), vp(d_bg), C.byref(H.PtFilmMapParams(full, mx, 2, H.SAMPLE_RNG, 0)), vp(d_budget), s)
assert add(3) == H.OK, lib.pt_last_error(ctx)
assert add_map(0) == H.ERR_ARGUMENT and add_map(4097) == H.ERR_ARGUMENT
assert add_map(12) == H.OK, lib.pt_last_error(ctx)
# refused while the pass is open, each with PT_ERR_ARGUMENT, the film unharmed
refine = H.PtFilmRefineParams(full, 0.0, 0, 64, 8)
assert add_map(12) == H.ERR_ARGUMENT and add(1) == H.ERR_ARGUMENT
assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(up)) == H.ERR_ARGUMENT
assert lib.pt_film_error(ctx, film, np.zeros((h, w)).ctypes.data_as(H._dp)) == H.ERR_ARGUMENT
assert lib.pt_film_budget_device(ctx, film, C.byref(refine), vp(t_out_budget), vp(t_summary), s) == H.ERR_ARGUMENT
assert lib.pt_film_reset(ctx, film) == H.ERR_ARGUMENT and lib.pt_film_destroy(ctx, film) == H.ERR_ARGUMENT
# queued behind the pass on its stream: they see its samples
assert lib.pt_film_resolve_device(ctx, film, vp(t_rgb), vp(t_lin), s) == H.OK
assert lib.pt_film_error_device(ctx, film, vp(t_err), s) == H.OK
ms = C.c_double(-1.0)
assert lib.pt_radiance_finish(ctx, C.byref(ms)) == H.OK and ms.value > 0.0
assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight any more
stream.synchronize()
assert t_rgb.cpu().numpy().tobytes() == ref_rgb.tobytes() and t_lin.cpu().numpy().tobytes() == ref_lin.tobytes()
assert t_err.cpu().numpy().tobytes() == ref_err.tobytes()
# the host's copy of the counts is 3 + 12 everywhere, an upper bound: an add that would pass 2^31 from THERE is refused, whatever the pixels really hold
most = int(ref_counts.max())
assert most == 15 and int(ref_counts.min()) == 3
assert add((1 << 31) - 15 + 1) == H.ERR_ARGUMENT and b"2^31" in lib.pt_last_error(ctx)
low = np.argwhere(ref_counts == 3)[0]
at_low = H.PtRect(int(low[1]), int(low[0]), int(low[1]), int(low[0]))
near = lambda rect, samples: lib.pt_film_add(ctx, film, C.byref(cam), bg.ctypes.data_as(H._dp), C.byref(H.PtFilmParams(rect, samples, 2, H.SAMPLE_RNG, 0)), None)
assert near(at_low, (1 << 31) - 15 + 1) == H.ERR_ARGUMENT, "a pixel that took nothing is still bounded by max_samples until the counts are read"
# pt_film_counts gives the device's values, and the refusals are what the header says for them
assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(up)) == H.OK and np.array_equal(counts, ref_counts)
assert near(at_low, (1 << 31) - 3 + 1) == H.ERR_ARGUMENT and b"2^31" in lib.pt_last_error(ctx)
assert add((1 << 31) - 15 + 1) == H.ERR_ARGUMENT and add((1 << 31) + 1) == H.ERR_ARGUMENT
assert lib.pt_film_counts(ctx, film, counts.ctypes.data_as(up)) == H.OK and np.array_equal(counts, ref_counts), "the refused adds left the film alone"
# the budget kernel and its summary, against numpy
refine = H.PtFilmRefineParams(H.PtRect(9, 5, 40, 30), float(np.median(ref_err[np.isfinite(ref_err)])), 4, 14, 8)
assert lib.pt_film_budget_device(ctx, film, C.byref(refine), vp(t_out_budget), vp(t_summary), s) == H.OK, lib.pt_last_error(ctx)
stream.synchronize()
c = ref_counts.astype(np.int64)
want = np.where(c < 4, np.minimum(4 - c, 8), np.where((c < 14) & (ref_err > refine.threshold), np.minimum(8, 14 - c), 0))
inside = np.zeros((h, w), dtype=bool); inside[5:31, 9:41] = True
want = np.where(inside, want, 0)
got = t_out_budget.cpu().numpy().view(np.uint32)
assert np.array_equal(got, want) and (want > 0).any() and (want[inside] == 0).any() and len(np.unique(want)) > 2
assert t_summary.cpu().numpy().tolist() == [int((want > 0).sum()), int(want.sum())]
assert lib.pt_film_destroy(ctx, film) == H.OK
# a plain film has no error and no budget
assert lib.pt_film_create(ctx, w, h, C.byref(film)) == H.OK
assert lib.pt_film_error_device(ctx, film, vp(t_err), s) == H.ERR_ARGUMENT and lib.pt_film_error(ctx, film, np.zeros((h, w)).ctypes.data_as(H._dp)) == H.ERR_ARGUMENT
assert lib.pt_film_budget_device(ctx, film, C.byref(refine), vp(t_out_budget), vp(t_summary), s) == H.ERR_ARGUMENT
assert lib.pt_film_destroy(ctx, film) == H.OK
r.close()
assert (x * 2).sum().item() == 2048.0
print("a device map into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "a device map into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 4. the plan kernels
def scan_levels(n_slots):
    """Levels of block sums the plan needs: one per factor of PLAN_BLOCK, until one block can scan what is left."""
    levels, k = 0, n_slots
    while True:
        k = -(-k // PLAN_BLOCK)
        levels += 1
        if k <= PLAN_BLOCK:
            return levels


def slots_of(side):
    return (-(-side // 8)) ** 2 * 64


def test_the_plan_kernels_write_the_host_replays_list(H):
    """A plan alone launches no sampling. 67 x 37 has 45 tiles = 2880 slots = 12 blocks of 256: one level of sums, scanned by one block. One more level is needed
    from 257 blocks on, more than 65536 slots = 1024 tiles: a square film needs 33 x 33 tiles, a side of 257."""
    assert scan_levels(45 * 64) == 1
    side = next(s for s in range(1, 2000) if scan_levels(slots_of(s)) == 2)
    assert side == 257 and slots_of(256) == PLAN_BLOCK * PLAN_BLOCK and scan_levels(slots_of(256)) == 1
    lib = H.lib()
    ctx = H.Context()  # no scene, no film
    for (w, h), rects in (((W, HT), [(0, 0, W - 1, HT - 1), RECT, (33, 17, 33, 17)]), ((side, side), [(0, 0, side - 1, side - 1), (3, 5, side - 2, side - 7)])):
        budget = BUDGETS[np.random.default_rng(w).integers(0, len(BUDGETS), size=(h, w))]
        longest = 0
        for rect in rects:
            for rnd, mx in ((0, 17), (1, 17), (2, 17), (0, 5), (1, 9)):
                want, n_want, _ = host_plan(H, w, h, rect, budget, mx, rnd)
                cap = max(n_want, 1)
                lst = np.full(cap, 0xFFFFFFFF, dtype=np.uint32)
                n = C.c_uint32(0xFFFFFFFF)
                rc = lib.pt_test_film_plan(ctx.handle, w, h, C.byref(H.PtRect(*rect)), budget.ctypes.data_as(H._up), mx, rnd, lst.ctypes.data_as(H._up), cap, C.byref(n))
                assert rc == H.OK, lib.pt_last_error(ctx.handle)
                assert n.value == n_want and np.array_equal(lst[:n_want], want), ((w, h), rect, rnd, mx)
                longest = max(longest, n_want)
        assert longest > 3 * w * h, "some list of this film must be long enough to mean something"
    zeros = np.zeros((HT, W), dtype=np.uint32)
    n = C.c_uint32(7)
    assert lib.pt_test_film_plan(ctx.handle, W, HT, C.byref(H.PtRect(0, 0, W - 1, HT - 1)), zeros.ctypes.data_as(H._up), 8, 0, None, 0, C.byref(n)) == H.OK and n.value == 0
    ctx.close()


# ---- 5. moments and error
def numpy_film(values):
    """(n, H, W, 3) per-sample values -> (sum as DESIGN section 2 associates it, q, err as include/portrayer_hip.h states it), one rounding per operation."""
    n = len(values)
    chunks = []
    for k in range(0, n, 8):
        c = values[k].copy()
        for v in values[k + 1:k + 8]:
            c = c + v
        chunks.append(c)
    S = chunks[0]
    for c in chunks[1:]:
        S = S + c
    q = None
    for v in values:
        y = (v[..., 0] + v[..., 1]) + v[..., 2]
        q = y * y if q is None else q + y * y
    dn = np.float64(n)
    mean = S / dn
    my = (mean[..., 0] + mean[..., 1]) + mean[..., 2]
    var = (q - (dn * my) * my) / np.float64(n - 1)
    var = np.where(var > 0.0, var, 0.0)
    return S, q, np.sqrt(var / dn)


@pytest.mark.parametrize("name,mode_name", [("soft-shadows", "SAMPLE_CENTRE"), ("glossy-reflection", "SAMPLE_RNG")])
def test_the_error_is_the_numpy_restatement_over_the_films_own_samples(oracle, host, H, name, mode_name):
    """11 samples in adds of 3, 5 and 3. The per-sample values come from Renderer.radiance over the film's own primary rays (stream = the pixel, sample = s,
    the background per ray). FIRST they are shown to be the film's samples - folded by numpy as section 2 folds them they give the film's linear, bit for bit -
    THEN error() must equal the restatement over them."""
    sample_mode = getattr(H, mode_name)
    scene, cam, _ = all_examples()[name]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(6).uniform(0.0, 1.0, size=(HT, W, 3))
    ys, xs = np.mgrid[0:HT, 0:W]
    pixel = (ys * W + xs).ravel()
    seed, n = 7, 11
    rays = []  # the film's primary rays, sample by sample: the same for every traversal
    for s in range(n):
        if sample_mode == H.SAMPLE_CENTRE:
            jx = jy = np.full(len(pixel), 0.5)
        else:
            jx = np.array([oracle.rng_draw(seed, int(p), s, 0) for p in pixel])
            jy = np.array([oracle.rng_draw(seed, int(p), s, 1) for p in pixel])
        rays.append(oracle.camera_rays(cam, W, HT, np.stack([xs.ravel() + jx, ys.ravel() + jy], axis=1)))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        film = r.film(W, HT, moments=True)
        for k in (3, 5, 3):
            film.add(c10, bg, samples=k, seed=seed, sample_mode=sample_mode)
        values = [r.radiance(o, d, background=bg.reshape(-1, 3), seed=seed, sample=s, stream_base=0)["rgb"].reshape(HT, W, 3) for s, (o, d) in enumerate(rays)]
        S, q, err = numpy_film(np.array(values))
        linear = film.resolve()[1]
        assert np.array_equal(bits(S / np.float64(n)), bits(linear)), "%s %s: the radiance values are not the film's samples" % (name, mname)
        got = film.error()
        assert np.array_equal(bits(got), bits(err)), "%s %s: error() differs from the restatement at %d pixels" % (name, mname, int((bits(got) != bits(err)).sum()))
        assert np.isfinite(got).all() and (got > 0.0).any()
        film.close()
        r.close()


def test_counts_below_two_have_no_error_and_a_plain_film_has_none(oracle, host, H):
    scene, cam, _ = all_examples()["soft-shadows"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(6).uniform(0.0, 1.0, size=(HT, W, 3))
    r = host.Renderer(hs, H.TRAVERSE_FLAT, kd_depth=8)
    film = r.film(W, HT, moments=True)
    assert np.isposinf(film.error()).all()
    budget = np.zeros((HT, W), dtype=np.uint32)
    budget[:, :30], budget[:, 30:50] = 1, 2
    film.add_map(c10, bg, budget, seed=7, sample_mode=H.SAMPLE_RNG)
    e = film.error()
    assert np.isposinf(e[:, :30]).all() and np.isfinite(e[:, 30:50]).all() and np.isposinf(e[:, 50:]).all()
    film.reset()
    assert np.isposinf(film.error()).all()
    plain = r.film(W, HT)
    with pytest.raises(ValueError, match="moments"):
        plain.error()
    with pytest.raises(ValueError, match="moments"):
        plain.refine(c10, bg, 0.01)
    film.close(); plain.close()
    r.close()


# ---- 6. refine
def test_refine_is_the_loop_numpy_drives_and_every_pixel_its_render(oracle, host, H):
    """min_count = step = 8, max_count = 32; the threshold is measured: the median of the positive errors after 8 samples. The second film is driven from the
    host: error() after each pass, the budget rule restated in numpy, add_map."""
    scene, cam, _ = all_examples()["soft-shadows"]()
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    bg = np.random.default_rng(8).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, _ in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        probe = r.film(W, HT, moments=True)
        probe.add(c10, bg, samples=8, seed=7, sample_mode=H.SAMPLE_RNG)
        e8 = probe.error()
        threshold = float(np.median(e8[e8 > 0.0]))
        probe.close()
        film = r.film(W, HT, moments=True)
        out = film.refine(c10, bg, threshold, min_count=8, max_count=32, step=8, max_passes=16, seed=7, sample_mode=H.SAMPLE_RNG)
        counts = film.counts()
        assert set(int(v) for v in np.unique(counts)) <= {8, 16, 24, 32}
        assert (counts == 8).any() and (counts > 8).any(), "both 'stayed at 8' and 'got more' must occur"
        assert out["samples"] == int(counts.sum()) and out["pixels_left"] == 0 and 2 <= out["passes"] <= 4 and out["kernel_ms"] > 0.0
        by_hand = r.film(W, HT, moments=True)
        passes = 0
        while True:
            c, e = by_hand.counts().astype(np.int64), by_hand.error()
            budget = np.where(c < 8, np.minimum(8 - c, 8), np.where((c < 32) & (e > threshold), np.minimum(8, 32 - c), 0)).astype(np.uint32)
            if not budget.any():
                break
            by_hand.add_map(c10, bg, budget, seed=7, sample_mode=H.SAMPLE_RNG, max_samples=8)
            passes += 1
        assert passes == out["passes"] and np.array_equal(by_hand.counts(), counts)
        got = film.resolve()
        same_image(by_hand.resolve(), got, "soft-shadows %s: refine vs the loop driven from the host" % mname)
        assert np.array_equal(bits(by_hand.error()), bits(film.error()))
        each_count_is_its_render(r, H, c10, bg, got, counts, 7, H.SAMPLE_RNG, "soft-shadows %s after refine" % mname)
        # max_passes: one pass brings every pixel to 8 and reports who still wants more
        film.reset()
        first = film.refine(c10, bg, threshold, min_count=8, max_count=32, step=8, max_passes=1, seed=7, sample_mode=H.SAMPLE_RNG)
        assert first["passes"] == 1 and first["samples"] == 8 * W * HT and np.all(film.counts() == 8) and first["pixels_left"] == int((e8 > threshold).sum())
        film.close(); by_hand.close()
        r.close()
