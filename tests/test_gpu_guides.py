"""The guides pass (pt_guides / pt_guides_device / Renderer.guides) on the device: the albedo against the oracle, bit for bit, and position,
normal and node against Renderer.aov's bits.

The albedo's oracle: the scene with no light, ambient (1, 1, 1) and every material's reflectivity 0, its pixel-centre rays coloured over a black background -
1.0 * diffuse_color and nothing else (material.rs:148, :216), +0 where nothing is hit. Sphere texture coordinates go through atan2 / acos, which the device
evaluates within 2 / 1 ulp of glibc's, so such a scene is exact only where no lookup comes near a texel edge - which the oracle's render counts
(tests/test_gpu_textures.py::texel_edge_proof) and this file asserts for every scene and size it uses. There is no tolerance in this file. 67 x 37 unless said."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37  # a multiple of 8 in neither direction
ALL = ("albedo", "position", "normal", "node")
EXAMPLES = ["texture-mapping", "normal-mapping", "cube-mapping", "transmission-refraction", "primitives", "macho-cows"]
GENERATED = ["textured:1", "random:3"]
KD_DEPTH = 8


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
    """The golden assets plus a stand-in for earth_cube.png, which texture-mapping and cube-mapping open and the reference repository lacks
    (tests/test_examples_extra.py)."""
    from PIL import Image
    d = tmp_path_factory.mktemp("assets")
    for f in os.listdir(ASSETS):
        os.symlink(os.path.join(ASSETS, f), os.path.join(d, f))
    Image.fromarray(np.random.default_rng(3).integers(0, 256, size=(48, 64, 3), dtype=np.uint8)).save(os.path.join(d, "earth_cube.png"))
    return str(d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def modes(H, O):
    return {"flat": (H.TRAVERSE_FLAT, O.MODE_FLAT), "kd": (H.TRAVERSE_KD, O.MODE_KD), "hier": (H.TRAVERSE_HIER, O.MODE_HIER)}


def load(host, O, which, assets):
    """(the host library's scene, its 10 camera numbers, the oracle's arrays of it) of an example scene or of a scene_dsl generated one."""
    if ":" not in which:
        sc = host.Scene.example(which, assets=assets)
        return sc, sc.camera, sc.export()
    kind, seed = which.split(":")
    if kind == "textured":
        from test_gpu_textures import textured_scene
        scene, cam = textured_scene(int(seed))
    else:
        from test_gpu_render_parity import random_scene
        scene, cam = random_scene(int(seed))
    return host_glue.host_scene(scene), host_glue.cam10(cam), O.pack(scene).arrays


def albedo_scene(O, arrays):
    """The oracle scene whose colour IS the albedo: no light, ambient (1, 1, 1), no reflectivity."""
    a = dict(arrays)
    a["n_lights"] = 0
    a["ambient"] = (1.0, 1.0, 1.0)
    m = np.array(a["materials"], dtype=np.float64, copy=True)
    m[:, 7] = 0.0
    a["materials"] = m
    return O.pack_arrays(a)


def oracle_albedo(O, ps, cam, w, h, mode, offset=(0.5, 0.5), rect=None):
    """(h, w, 3): camera_rays then color_rays over a black background, for the pixels of rect (default: the image). At the pixel centres the oracle's render of
    one centre sample must say the same and count no sphere lookup near a texel edge."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w - 1, h - 1)
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    xy = np.stack([xs.ravel() + offset[0], ys.ravel() + offset[1]], axis=1).astype(np.float64)
    o, d = O.camera_rays(cam, w, h, xy)
    col = O.color_rays(ps, o, d, (0.0, 0.0, 0.0), mode=mode, kd_depth=KD_DEPTH).reshape(y1 - y0 + 1, x1 - x0 + 1, 3)
    if tuple(offset) == (0.5, 0.5) and rect is None:
        ref = O.render(ps, cam, w, h, background=np.zeros((h, w, 3)), samples=1, jitter=O.JITTER_CENTRE, mode=mode, kd_depth=KD_DEPTH)
        assert ref.stats["tex_sphere_near_edge"] == 0, "a sphere's texture coordinate lies within 4096 ulps of a texel edge: pick another scene / size for this test"
        assert np.array_equal(bits(ref.linear), bits(col)), "the oracle's render of one centre sample != its color_rays"
    return col


# ---- 1. the albedo against the oracle; position, normal and node against the aov pass
@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
@pytest.mark.parametrize("which", EXAMPLES + GENERATED)
def test_albedo_equals_the_oracle_and_the_rest_equals_the_aov_pass(oracle, host, H, assets, which, mode):
    sc, cam, arrays = load(host, oracle, which, assets)
    tr, om = modes(H, oracle)[mode]
    want = oracle_albedo(oracle, albedo_scene(oracle, arrays), cam, W, HT, om)
    r = host.Renderer(sc, tr, kd_depth=KD_DEPTH)
    got = r.guides(cam, W, HT)
    aov = r.aov(cam, W, HT, want=("position", "normal", "node"))
    r.close()
    hit = got["node"] >= 0
    differ = (bits(got["albedo"]) != bits(want)).any(axis=-1)
    print("%s %s: %d of %d pixels differ (%d hits, %d distinct colours)" % (which, mode, int(differ.sum()), differ.size, int(hit.sum()), len(np.unique(want.reshape(-1, 3), axis=0))))
    assert hit.sum() > 500 and ((~hit).any() or which == "transmission-refraction"), "the camera must see the scene and - except inside transmission-refraction's closed room - some background"
    assert np.array_equal(bits(got["albedo"]), bits(want)), "%s %s: albedo differs from the oracle's at %r" % (which, mode, np.argwhere(differ)[:3].tolist())
    assert not bits(got["albedo"])[~hit].any(), "misses must hold +0"
    for k in ("position", "normal", "node"):
        assert got[k].tobytes() == aov[k].tobytes(), "%s %s: %s differs from the aov pass's" % (which, mode, k)
    if which in ("texture-mapping", "textured:1", "transmission-refraction"):
        assert len(np.unique(want.reshape(-1, 3), axis=0)) > 50, "the scene must show texture"


# ---- 2. offset, sizes, slices, single buffers
@pytest.mark.parametrize("which,mode", [("primitives", "hier"), ("cube-mapping", "flat"), ("macho-cows", "kd")])
def test_offset_other_than_the_pixel_centre(oracle, host, H, assets, which, mode):
    """(No scene with a textured sphere: away from the centre the oracle's render cannot vouch for the texel edges.)"""
    sc, cam, arrays = load(host, oracle, which, assets)
    tr, om = modes(H, oracle)[mode]
    offset = (0.25, 0.8125)
    want = oracle_albedo(oracle, albedo_scene(oracle, arrays), cam, W, HT, om, offset=offset)
    r = host.Renderer(sc, tr, kd_depth=KD_DEPTH)
    got = r.guides(cam, W, HT, offset=offset)
    centre = r.guides(cam, W, HT, want=("position",))
    aov = r.aov(cam, W, HT, offset=offset, want=("position", "normal", "node"))
    r.close()
    assert np.array_equal(bits(got["albedo"]), bits(want))
    assert got["position"].tobytes() != centre["position"].tobytes(), "the offset must move the rays"
    for k in ("position", "normal", "node"):
        assert got[k].tobytes() == aov[k].tobytes(), k


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
def test_a_one_by_one_image(oracle, host, H, assets, mode):
    sc, cam, arrays = load(host, oracle, "textured:1", assets)  # (its centre pixel is on a textured surface)
    tr, om = modes(H, oracle)[mode]
    want = oracle_albedo(oracle, albedo_scene(oracle, arrays), cam, 1, 1, om)
    r = host.Renderer(sc, tr, kd_depth=KD_DEPTH)
    got = r.guides(cam, 1, 1)
    aov = r.aov(cam, 1, 1, want=("position", "normal", "node"))
    r.close()
    assert got["node"][0, 0] >= 0 and want.any(), "the centre of the image must hit the scene"
    assert np.array_equal(bits(got["albedo"]), bits(want)) and all(got[k].tobytes() == aov[k].tobytes() for k in ("position", "normal", "node"))


@pytest.mark.parametrize("which,mode", [("texture-mapping", "flat"), ("transmission-refraction", "hier"), ("primitives", "kd")])
def test_a_rectangle_off_the_tile_grid_leaves_everything_outside_untouched(host, H, assets, which, mode):
    sc, cam, _ = load(host, None, which, assets)
    r = host.Renderer(sc, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mode], kd_depth=KD_DEPTH)
    full = r.guides(cam, W, HT)
    rect = (3, 5, 15, 15)  # 13 x 11 pixels at (3, 5): no corner on a tile boundary
    into = {k: np.full((HT, W) + ((3,) if n == 3 else ()), -7 if dt is np.int32 else -7.25, dtype=dt) for k, (dt, n) in H.GUIDES_BUFFERS.items()}
    sentinel = {k: v.copy() for k, v in into.items()}
    part = r.guides(cam, W, HT, rect=rect, into=into)
    inside = np.zeros((HT, W), dtype=bool)
    inside[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1] = True
    assert (full["node"][inside] >= 0).any()
    for k in ALL:
        assert part[k] is into[k]
        assert part[k][inside].tobytes() == full[k][inside].tobytes(), "%s: inside the slice != the full frame" % k
        assert part[k][~inside].tobytes() == sentinel[k][~inside].tobytes(), "%s: a pixel outside the slice was written" % k
    r.close()


@pytest.mark.parametrize("which,mode", [("normal-mapping", "hier"), ("transmission-refraction", "flat"), ("macho-cows", "kd")])
def test_every_single_buffer_request_equals_the_all_buffers_request(host, H, assets, which, mode):
    sc, cam, _ = load(host, None, which, assets)
    r = host.Renderer(sc, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mode], kd_depth=KD_DEPTH)
    full = r.guides(cam, W, HT)
    assert set(full) == set(ALL) | {"kernel_ms"}
    for k in ALL:
        one = r.guides(cam, W, HT, want=(k,))
        assert set(one) == {k, "kernel_ms"}
        assert one[k].tobytes() == full[k].tobytes(), k
    two = r.guides(cam, W, HT, want=("albedo", "node"))
    assert two["albedo"].tobytes() == full["albedo"].tobytes() and two["node"].tobytes() == full["node"].tobytes()
    r.close()


def test_argument_errors(host, H):
    lib = H.lib()
    sc = host.Scene.example("primitives", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ctx = r.context
    cam = host.camera(sc.camera, W, HT)
    albedo = np.zeros((HT, W, 3))
    b = H.PtGuidesBuffers(albedo=albedo.ctypes.data_as(H._dp))
    good = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_guides(ctx, C.byref(cam), C.byref(good), C.byref(b), None) == H.OK and albedo.any()
    for rect in ((0, 0, W, HT - 1), (0, 0, W - 1, HT), (W, 0, W - 1, HT - 1), (0, HT, W - 1, HT - 1)):
        p = H.PtAovParams(W, HT, H.PtRect(*rect), (C.c_double * 2)(0.5, 0.5))
        assert lib.pt_guides(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_SLICE, rect
        assert lib.pt_guides_device(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_SLICE, rect
    with pytest.raises(host.PortrayerPanic):
        r.guides(sc.camera, W, HT, rect=(0, 0, W, HT - 1))
    assert lib.pt_guides(ctx, C.byref(cam), None, C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_guides(ctx, None, C.byref(good), C.byref(b), None) == H.ERR_ARGUMENT
    assert lib.pt_guides(ctx, C.byref(cam), C.byref(good), C.byref(H.PtGuidesBuffers()), None) == H.ERR_ARGUMENT and b"no output buffer" in lib.pt_last_error(ctx)
    assert lib.pt_guides(ctx, C.byref(cam), C.byref(good), None, None) == H.ERR_ARGUMENT
    for off in ((float("nan"), 0.5), (0.5, float("inf"))):
        p = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(*off))
        assert lib.pt_guides(ctx, C.byref(cam), C.byref(p), C.byref(b), None) == H.ERR_ARGUMENT, off
    assert lib.pt_guides_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    bare = H.Context()
    assert lib.pt_guides(bare.handle, C.byref(cam), C.byref(good), C.byref(b), None) == H.ERR_NO_SCENE
    assert lib.pt_guides_device(bare.handle, C.byref(cam), C.byref(good), C.byref(b), None) == H.ERR_NO_SCENE
    bare.close()
    empty = H.PtAovParams(W, HT, H.PtRect(5, 5, 4, 4), (C.c_double * 2)(0.5, 0.5))  # an inverted slice traces nothing
    albedo[:] = 3.0
    assert lib.pt_guides(ctx, C.byref(cam), C.byref(empty), C.byref(b), None) == H.OK and np.all(albedo == 3.0)
    r.close()


# ---- 3. device buffers, and the pass the two kinds share
def test_device_buffers_on_a_stream_equal_the_host_path_and_the_two_passes_exclude_each_other(H, assets):
    """pt_guides_device into torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first (as in
    tests/test_gpu_aov.py). A guides pass while an aov pass is open is refused, and the reverse; either finish call closes whichever is open."""
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
W, HT = 67, 37
lib = H.lib()
sc = host.Scene.example("texture-mapping", assets=%r)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
ctx = r.context
ref = r.guides(sc.camera, W, HT)
ref_aov = r.aov(sc.camera, W, HT, want=("depth",))
assert (ref["node"] >= 0).sum() > 500 and len(np.unique(ref["albedo"].reshape(-1, 3), axis=0)) > 50
cam = host.camera(sc.camera, W, HT)
p = H.PtAovParams(W, HT, H.PtRect(0, 0, W - 1, HT - 1), (C.c_double * 2)(0.5, 0.5))
t = {k: torch.full((HT, W) + ((3,) if n == 3 else ()), -5, dtype=torch.float64 if dt is np.float64 else torch.int32, device=dev) for k, (dt, n) in H.GUIDES_BUFFERS.items()}
t_depth = torch.full((HT, W), -5, dtype=torch.float64, device=dev)
torch.cuda.synchronize()
stream = torch.cuda.Stream(device=dev)
assert stream.cuda_stream != 0
s = C.c_void_p(stream.cuda_stream)
b = H.PtGuidesBuffers()
for k, (dt, _) in H.GUIDES_BUFFERS.items():
    setattr(b, k, C.cast(C.c_void_p(t[k].data_ptr()), H._dp if dt is np.float64 else H._ip))
ab = H.PtAovBuffers(depth=C.cast(C.c_void_p(t_depth.data_ptr()), H._dp))
host_depth = np.full((HT, W), 7.0)
hb = H.PtAovBuffers(depth=host_depth.ctypes.data_as(H._dp))
host_albedo = np.full((HT, W, 3), 7.0)
hg = H.PtGuidesBuffers(albedo=host_albedo.ctypes.data_as(H._dp))
ms = C.c_double(-1.0)
# a guides pass open: a second one, and an aov pass in either form, are refused
assert lib.pt_guides_device(ctx, C.byref(cam), C.byref(p), C.byref(b), s) == H.OK, lib.pt_last_error(ctx)
assert lib.pt_guides_device(ctx, C.byref(cam), C.byref(p), C.byref(b), s) == H.ERR_ARGUMENT and b"in flight" in lib.pt_last_error(ctx)
assert lib.pt_aov_device(ctx, C.byref(cam), C.byref(p), C.byref(ab), s) == H.ERR_ARGUMENT and b"in flight" in lib.pt_last_error(ctx)
assert lib.pt_aov(ctx, C.byref(cam), C.byref(p), C.byref(hb), None) == H.ERR_ARGUMENT and (host_depth == 7.0).all()
assert lib.pt_guides(ctx, C.byref(cam), C.byref(p), C.byref(hg), None) == H.ERR_ARGUMENT and (host_albedo == 7.0).all()
assert lib.pt_guides_finish(ctx, C.byref(ms)) == H.OK and ms.value > 0.0
assert lib.pt_guides_finish(ctx, None) == H.ERR_ARGUMENT and lib.pt_aov_finish(ctx, None) == H.ERR_ARGUMENT
stream.synchronize()
for k in H.GUIDES_BUFFERS:
    assert t[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
assert (t_depth.cpu().numpy() == -5).all(), "a refused pass writes nothing"
# an aov pass open: a guides pass is refused; pt_guides_finish closes it (the same function on the same pass)
assert lib.pt_aov_device(ctx, C.byref(cam), C.byref(p), C.byref(ab), s) == H.OK, lib.pt_last_error(ctx)
for k in t:
    t[k].fill_(-5)
assert lib.pt_guides_device(ctx, C.byref(cam), C.byref(p), C.byref(b), s) == H.ERR_ARGUMENT and b"in flight" in lib.pt_last_error(ctx)
assert lib.pt_guides(ctx, C.byref(cam), C.byref(p), C.byref(hg), None) == H.ERR_ARGUMENT and (host_albedo == 7.0).all()
assert lib.pt_guides_finish(ctx, None) == H.OK
stream.synchronize()
assert t_depth.cpu().numpy().tobytes() == ref_aov["depth"].tobytes()
assert all((t[k].cpu().numpy() == -5).all() for k in t), "a refused pass writes nothing"
# and through pt_aov_finish
assert lib.pt_guides_device(ctx, C.byref(cam), C.byref(p), C.byref(b), s) == H.OK, lib.pt_last_error(ctx)
assert lib.pt_aov_finish(ctx, None) == H.OK
stream.synchronize()
for k in H.GUIDES_BUFFERS:
    assert t[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
r.close()
assert (x * 2).sum().item() == 2048.0
print("guides into torch tensors ok")
""" % (root, root, assets)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "guides into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_renders_around_and_in_flight_across_a_pass_are_unchanged(host, H):
    w, h, samples = 96, 56, 2
    bg = default_background(w, h)
    sc = host.Scene.example("macho-cows", assets=ASSETS)
    r1, r2 = host.Renderer(sc, H.TRAVERSE_FLAT), host.Renderer(sc, H.TRAVERSE_FLAT)
    a1 = r1.render(sc.camera, w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG)
    r1.guides(sc.camera, W, HT)
    b1 = r1.render(sc.camera, w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG)
    a2 = r2.render(sc.camera, w, h, bg, samples=samples, seed=3, sample_mode=H.SAMPLE_RNG)
    b2 = r2.render(sc.camera, w, h, bg, samples=samples, seed=4, sample_mode=H.SAMPLE_RNG)  # this renderer never ran a pass
    for (x, y) in ((a1, a2), (b1, b2)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    # pt_render_device x 2 in flight, a guides pass, pt_render_finish x 2: the images of the renderer that never ran a pass
    want = [r2.render(sc.camera, w, h, bg, samples=samples, seed=10 + k, sample_mode=H.SAMPLE_RNG)[0] for k in range(2)]
    ref = r2.guides(sc.camera, w, h)
    lib, c = H.lib(), r1.context
    camera = host.camera(sc.camera, w, h)
    d_bg = C.c_void_p()
    assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
    d_img = [C.c_void_p(), C.c_void_p()]
    rows = 1 if bg.shape == (h, 3) else 0
    for k in range(2):
        assert lib.pt_device_alloc(c, w * h * 3, C.byref(d_img[k])) == 0
        p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, rows, 0, 1, 0)
        assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img[k], C.c_void_p(lib.pt_context_stream(c, k))) == 0, lib.pt_last_error(c)
    out = {k: np.zeros((h, w) + ((3,) if n == 3 else ()), dtype=dt) for k, (dt, n) in H.GUIDES_BUFFERS.items()}
    b = H.PtGuidesBuffers(**{k: out[k].ctypes.data_as(H._dp if dt is np.float64 else H._ip) for k, (dt, _) in H.GUIDES_BUFFERS.items()})
    gp = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
    assert lib.pt_guides(c, C.byref(camera), C.byref(gp), C.byref(b), None) == H.OK, lib.pt_last_error(c)
    for k in ALL:
        assert out[k].tobytes() == ref[k].tobytes(), k
    st = H.PtStats()
    for k in range(2):
        assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
        img = np.zeros((h, w, 3), dtype=np.uint8)
        assert lib.pt_copy_from_device(c, img.ctypes.data_as(C.c_void_p), d_img[k], img.nbytes) == 0
        assert np.array_equal(img, want[k]), "frame %d in flight across the pass differs from the render of a renderer that never ran one" % k
    for d in d_img + [d_bg]:
        lib.pt_device_free(c, d)
    r1.close(); r2.close()
