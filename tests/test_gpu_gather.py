"""The gather pass (pt_gather / pt_gather_device / Renderer.gather / Renderer.gather_camera) on the GPU, bit for bit.

The yardstick is the two passes that exist: the numpy restatement of the ambient-occlusion contract (tests/test_ao_contract.py, equal to the host replay in every
bit) makes each point's rays, Renderer.radiance - pinned to the oracle by tests/test_gpu_radiance.py - shades them, flattened point-major, with
stream_base = first_index * S and sample = pass_index, and numpy adds each point's S colours per channel in ascending k from zero; invalid points are zeros.
`sum` and `valid` are compared exactly: there is no tolerance anywhere in this file. The points are what Renderer.aov finds under a 67 x 37 image (2,479 points,
misses included: they are invalid points; 39 wavefronts at S = 16, the last one ragged), the normals turned towards the camera's eye. The background is not
black, so a ray that leaves the scene shows, and its components are dyadic, so "S x background" is one value however it is added up."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS  # noqa: E402
from test_ao_contract import restate  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37
NPTS = W * HT
SEED = 7
BG = (0.25, 0.5, 1.0)
TRAVERSALS = ("flat", "hier", "kd")
SCENES = ("big-scene", "macho-cows", "soft-shadows", "glossy-reflection", "transmission-refraction", "entering-the-mirror-dimension")
WANT = ("sum", "valid")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def traversal(H, mname):
    return {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[mname]


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for c in _CASES.values():
        c["r"].close()
    _CASES.clear()


def case(host, H, which, mname):
    """A renderer of the scene in one traversal, the points under its image and the camera's eye: made once, shared, never written to."""
    key = (which, mname)
    if key not in _CASES:
        sc = host.Scene.example(which, assets=ASSETS)
        r = host.Renderer(sc, traversal(H, mname), kd_depth=10)
        aov = r.aov(sc.camera, W, HT, want=("position", "normal", "node"))
        P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
        eye = np.array(list(host.camera(sc.camera, W, HT).eye))
        for a in (P, N, eye):
            a.setflags(write=False)
        _CASES[key] = dict(sc=sc, r=r, P=P, N=N, eye=eye, hit=aov["node"].ravel() >= 0, refs={})
    return _CASES[key]


def reference(r, P, N, S, seed=SEED, pas=0, first=0, bias=0.0, eye=None, bg=BG):
    """What the two contracts say, from the existing passes: (sum f64 (n, 3), valid u8 (n,))."""
    O, D, valid = restate(P, N, S, seed, pas, first, bias, eye)
    n = len(P)
    total = np.zeros((n, 3))
    if n:
        rgb = r.radiance(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), bg, seed=seed, sample=pas, stream_base=first * S)["rgb"].reshape(n, S, 3)
        with np.errstate(all="ignore"):
            for k in range(S):  # ascending k, left to right, from (0, 0, 0), per channel
                for ch in range(3):
                    total[:, ch] = total[:, ch] + rgb[:, k, ch]
    total[valid == 0] = 0.0
    return total, valid.astype(np.uint8)


def case_reference(c, S, pas=0, bias=0.0, seed=SEED):
    key = (S, pas, bias, seed)
    if key not in c["refs"]:
        ref = reference(c["r"], c["P"], c["N"], S, seed=seed, pas=pas, bias=bias, eye=c["eye"])
        for a in ref:
            a.setflags(write=False)
        c["refs"][key] = ref
    return c["refs"][key]


def check(tag, got, ref):
    total, valid = ref
    assert got["sum"].dtype == np.float64 and got["valid"].dtype == np.uint8
    assert np.array_equal(got["valid"], valid), f"{tag}: valid"
    bad = np.flatnonzero((bits(got["sum"]) != bits(total)).any(axis=-1))
    assert not len(bad), f"{tag}: sum differs at {len(bad)} of {len(total)} points, first {bad[:5]}: {got['sum'][bad[:5]]} != {total[bad[:5]]}"


def shaded(ref, S):
    """(valid points whose sum is not S x background in some channel, valid points)"""
    total, valid = ref
    miss = np.array(BG) * S  # (exact: dyadic components)
    return int(((total != miss[None, :]).any(axis=1) & (valid == 1)).sum()), int(valid.sum())


# ---- 1. parity with the existing passes: every scene, every traversal
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", SCENES)
def test_sum_and_valid_equal_the_radiance_pass_on_the_restated_rays(host, H, which, mname):
    c = case(host, H, which, mname)
    ref = case_reference(c, 16)
    some, valid = shaded(ref, 16)
    print(f"{which} {mname}: {valid} valid points of {NPTS}, {some} with a sum other than 16 x background")
    assert np.array_equal(ref[1], c["hit"].astype(np.uint8)), "aov's misses are the invalid points"
    assert some > 0 and np.all(np.isfinite(ref[0]))
    got = c["r"].gather(c["P"], c["N"], BG, samples=16, seed=SEED, eye=c["eye"], want=WANT)
    check(f"{which} {mname}", got, ref)
    assert np.array_equal(bits(got["mean"]), bits(ref[0] / 16.0)) and not got["mean"][ref[1] == 0].any() and got["kernel_ms"] > 0.0


@pytest.mark.parametrize("which", ["big-scene", "macho-cows", "robot-alarm-clock"])
def test_the_reference_is_neither_zeros_nor_the_background(host, H, which):
    """The guard is on the REFERENCE: a pass that wrote only zeros, or only S x background, could not equal it."""
    c = case(host, H, which, "flat")
    ref = case_reference(c, 16)
    some, valid = shaded(ref, 16)
    print(f"{which}: {some} of {valid} valid points have a sum other than 16 x background")
    assert valid > 1000 and 10 * some >= valid
    check(which, c["r"].gather(c["P"], c["N"], BG, samples=16, seed=SEED, eye=c["eye"], want=WANT), ref)


# ---- 2. sample counts, a bias, how a batch is cut
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_sample_counts_and_a_bias(host, H, mname):
    c = case(host, H, "big-scene", mname)
    for S, bias in ((1, 0.0), (4, 0.0), (64, 0.0), (8, 0.015625)):
        ref = case_reference(c, S, bias=bias)
        some, valid = shaded(ref, S)
        print(f"big-scene {mname} S={S} bias={bias}: {some} of {valid} valid points with a sum other than S x background")
        assert some > 0
        check(f"S={S} bias={bias}", c["r"].gather(c["P"], c["N"], BG, samples=S, bias=bias, seed=SEED, eye=c["eye"], want=WANT), ref)
    assert not np.array_equal(bits(case_reference(c, 8, bias=0.015625)[0]), bits(case_reference(c, 8)[0])), "the bias moves the origins"


def test_batch_sizes_cuts_and_an_empty_batch(host, H):
    c = case(host, H, "big-scene", "flat")
    r, P, N, eye = c["r"], c["P"], c["N"], c["eye"]
    start = int(np.flatnonzero(c["hit"])[0])  # (the image's first rows see the sky: start where the points are)
    run = lambda P, N, **kw: r.gather(P, N, BG, seed=SEED, eye=eye, want=WANT, **kw)
    whole = reference(r, P, N, 16, first=5000, eye=eye)
    check("2,479 points", run(P, N, samples=16, first_index=5000), whole)
    for n in (1, 3, 63, 65):
        check(f"n={n}", run(P[start:start + n].copy(), N[start:start + n].copy(), samples=16, first_index=5000 + start), tuple(a[start:start + n] for a in whole))
    for S in (1, 4, 64):  # a partial last wavefront at every group size
        ref = reference(r, P[start:start + 65], N[start:start + 65], S, first=start, eye=eye)
        check(f"n=65 S={S}", run(P[start:start + 65].copy(), N[start:start + 65].copy(), samples=S, first_index=start), ref)
    a = run(P[:1000].copy(), N[:1000].copy(), samples=16, first_index=5000)
    b = run(P[1000:].copy(), N[1000:].copy(), samples=16, first_index=6000)
    check("cut at 1,000", {k: np.concatenate([a[k], b[k]]) for k in WANT}, whole)
    shifted = run(P[1000:].copy(), N[1000:].copy(), samples=16, first_index=5000)
    assert not np.array_equal(bits(shifted["sum"]), bits(whole[0][1000:])), "first_index is part of the stream"
    empty = r.gather(np.zeros((0, 3)), np.zeros((0, 3)), BG, samples=16, want=WANT)
    assert empty["sum"].shape == (0, 3) and empty["mean"].shape == (0, 3) and empty["valid"].shape == (0,) and empty["kernel_ms"] == 0.0
    only = r.gather(P, N, BG, samples=16, seed=SEED, first_index=5000, eye=eye, want=("valid",))  # one buffer alone
    assert sorted(only) == ["kernel_ms", "valid"] and np.array_equal(only["valid"], whole[1])
    big = 1 << 60  # the 64-bit stream product: (first_index + i) * S is reduced modulo 2^64 only, as stream_base + i is
    check("first_index 2^60", run(P[start:start + 65].copy(), N[start:start + 65].copy(), samples=4, first_index=big),
          reference(r, P[start:start + 65], N[start:start + 65], 4, first=big, eye=eye))


# ---- 3. passes and seeds
def test_two_passes_differ_and_each_equals_its_reference(host, H):
    c = case(host, H, "macho-cows", "flat")
    refs = [case_reference(c, 16, pas=p) for p in (0, 1)]
    assert not np.array_equal(bits(refs[0][0]), bits(refs[1][0]))
    for p in (0, 1):
        check(f"pass {p}", c["r"].gather(c["P"], c["N"], BG, samples=16, seed=SEED, pass_index=p, eye=c["eye"], want=WANT), refs[p])


def test_the_seed_reaches_the_area_lights_draws(host, H):
    c = case(host, H, "soft-shadows", "flat")
    a, b = case_reference(c, 16), case_reference(c, 16, seed=SEED + 1)
    assert not np.array_equal(bits(a[0]), bits(b[0]))
    check("seed + 1", c["r"].gather(c["P"], c["N"], BG, samples=16, seed=SEED + 1, eye=c["eye"], want=WANT), b)


# ---- 4. invalid points inside wavefronts
@pytest.mark.parametrize("which,mname", [("macho-cows", "flat"), ("big-scene", "kd"), ("transmission-refraction", "hier")])
def test_invalid_points_report_zeros_and_change_no_neighbour(host, H, which, mname):
    c = case(host, H, which, mname)
    ref = case_reference(c, 16)
    P, N = c["P"].copy(), c["N"].copy()
    rng = np.random.default_rng(5)
    hit = np.flatnonzero(c["hit"])
    spoil = rng.choice(hit, size=len(hit) // 5, replace=False)  # scattered: nearly every wavefront holds some
    kind = np.arange(len(spoil)) % 5
    P[spoil[kind == 0], 1] = np.nan
    N[spoil[kind == 1]] = 0.0
    N[spoil[kind == 2], 2] = -np.inf
    P[spoil[kind == 3], 0] = 2e18
    P[spoil[kind == 4]], N[spoil[kind == 4]] = 0.0, 0.0  # what aov writes where nothing is hit
    want = [a.copy() for a in ref]
    for a in want:
        a[spoil] = 0
    got = c["r"].gather(P, N, BG, samples=16, seed=SEED, eye=c["eye"], want=WANT)
    check(f"{which} {mname} with invalid points", got, want)
    assert not got["sum"][spoil].any() and not got["valid"][spoil].any() and want[0].any()
    nothing = c["r"].gather(np.full((130, 3), np.nan), np.ones((130, 3)), BG, samples=4, want=WANT)  # wavefronts without a single ray
    assert not nothing["sum"].any() and not nothing["valid"].any()


def test_a_ray_that_is_not_traced_reports_the_background(host, H):
    """Valid points whose origins a huge bias carries beyond 1e18: pt_radiance does not trace such a ray and answers its background; so does this pass."""
    c = case(host, H, "big-scene", "flat")
    first = np.flatnonzero(c["hit"])[:70]
    P, N = c["P"][first].copy(), c["N"][first].copy()
    ref = reference(c["r"], P, N, 8, bias=1e19, eye=c["eye"])
    assert np.all(ref[1] == 1) and np.array_equal(ref[0], np.tile(np.array(BG) * 8, (70, 1)))
    check("bias 1e19", c["r"].gather(P, N, BG, samples=8, bias=1e19, seed=SEED, eye=c["eye"], want=WANT), ref)
    N[::2] = 0.0  # ... and beside invalid points, which stay zeros
    got = c["r"].gather(P, N, BG, samples=8, bias=1e19, seed=SEED, eye=c["eye"], want=WANT)
    assert np.array_equal(got["valid"], np.arange(70) % 2) and not got["sum"][::2].any() and np.array_equal(got["sum"][1::2], ref[0][1::2])


# ---- 5. the camera form
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", ["big-scene", "transmission-refraction"])
def test_gather_camera_equals_gather_fed_with_the_aov_arrays(host, H, which, mname):
    c = case(host, H, which, mname)
    ref = case_reference(c, 16)
    got = c["r"].gather_camera(c["sc"].camera, W, HT, BG, samples=16, seed=SEED, want=WANT)
    assert got["sum"].shape == (HT, W, 3) and got["mean"].shape == (HT, W, 3) and got["valid"].shape == (HT, W) and got["kernel_ms"] > 0.0
    check(f"{which} {mname} gather_camera", {"sum": got["sum"].reshape(NPTS, 3), "valid": got["valid"].reshape(NPTS)}, ref)
    assert np.array_equal(got["valid"].ravel() == 1, c["hit"]), "miss pixels are invalid points"
    smaller = c["r"].gather_camera(c["sc"].camera, 16, 8, BG, samples=4)  # the renderer's scratch serves a smaller image after a larger one
    P8 = c["r"].aov(c["sc"].camera, 16, 8, want=("position", "normal"))
    eye8 = np.array(list(host.camera(c["sc"].camera, 16, 8).eye))
    again = c["r"].gather(P8["position"].reshape(-1, 3), P8["normal"].reshape(-1, 3), BG, samples=4, eye=eye8)
    assert np.array_equal(bits(smaller["sum"]).reshape(-1, 3), bits(again["sum"]))
    ao = c["r"].ao_camera(c["sc"].camera, W, HT, samples=16, seed=SEED, want=("occluded", "valid"))  # the ambient-occlusion form shares that scratch: still right
    assert np.array_equal(ao["valid"], got["valid"])


# ---- 6. parked frames in HBM
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_without_parked_frames_in_lds_the_bits_are_the_same(monkeypatch, host, H, mname):
    c = case(host, H, "transmission-refraction", mname)
    ref = case_reference(c, 16)  # (made with the default: frames parked in LDS)
    monkeypatch.setenv("PORTRAYER_PARK", "0")
    check(f"PORTRAYER_PARK=0 {mname}", c["r"].gather(c["P"], c["N"], BG, samples=16, seed=SEED, eye=c["eye"], want=WANT), ref)
    assert np.array_equal(bits(reference(c["r"], c["P"][:500], c["N"][:500], 16, eye=c["eye"])[0]), bits(ref[0][:500])), "the radiance pass agrees with itself, too"


# ---- 7. a moved scene
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_after_an_update_the_pass_answers_for_the_moved_scene(host, H, mname):
    from test_gpu_update import grid
    scene_a, cam_a, _ = grid(40, 0.0)()
    scene_b, cam_b, _ = grid(40, 0.7)()
    ha, hb, cam = host_glue.host_scene(scene_a), host_glue.host_scene(scene_b), host_glue.cam10(cam_b)
    r = host.Renderer(ha, traversal(H, mname), kd_depth=8)
    before = r.gather_camera(cam, W, HT, BG, samples=16, seed=SEED, want=WANT)
    r.update(hb)
    fresh = host.Renderer(hb, traversal(H, mname), kd_depth=8)
    moved, want = r.gather_camera(cam, W, HT, BG, samples=16, seed=SEED, want=WANT), fresh.gather_camera(cam, W, HT, BG, samples=16, seed=SEED, want=WANT)
    for k in WANT:
        assert moved[k].tobytes() == want[k].tobytes(), k
    aov = fresh.aov(cam, W, HT, want=("position", "normal"))
    eye = np.array(list(host.camera(cam, W, HT).eye))
    ref = reference(fresh, aov["position"].reshape(-1, 3), aov["normal"].reshape(-1, 3), 16, eye=eye)
    check(f"moved grid {mname}", {"sum": want["sum"].reshape(NPTS, 3), "valid": want["valid"].reshape(NPTS)}, ref)
    assert shaded(ref, 16)[0] > 0 and before["sum"].tobytes() != want["sum"].tobytes()
    r.close()
    fresh.close()


# ---- 8. device buffers, and the pass among the others
def test_device_tensors_on_a_torch_stream_among_renders_and_a_rays_pass(H):
    """pt_gather_device with points and results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first.
    While it is open a second radiance, film or gather pass is refused; a render on each slot and a rays pass are in flight around it, and everything equals what
    the same calls gave one after the other."""
    import subprocess
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
from scene_dsl import ASSETS, default_background
lib = H.lib()
sc = host.Scene.example("macho-cows", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
cx = r.context
aov = r.aov(sc.camera, 67, 37, want=("position", "normal"))
P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
n = len(P)
eye = list(host.camera(sc.camera, 67, 37).eye)
bg3 = np.array([0.25, 0.5, 1.0])
ref = r.gather(P, N, bg3, samples=16, seed=7, pass_index=2, first_index=11, eye=eye, want=("sum", "valid"))
miss = (ref["sum"] == bg3[None, :] * 16).all(axis=1)
assert ref["valid"].sum() > 1000 and 0 < (~miss & (ref["valid"] == 1)).sum()
w, h = 160, 96
cam = host.camera(sc.camera, w, h)
bg = default_background(w, h)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_P, d_N, d_bg = t(P), t(N), t(bg)
ptr = lambda tensor: C.c_void_p(tensor.data_ptr())
dp = lambda a: a.ctypes.data_as(H._dp)
film = C.c_void_p()
assert lib.pt_film_create(cx, w, h, C.byref(film)) == H.OK
p = H.PtGatherParams(n, 16, 2, 7, 11, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
rp = H.PtRaysParams(n, 1, 0)
results = []
for overlapped in (False, True):
    t_sum = torch.full((n, 3), 5.0, dtype=torch.float64, device=dev)
    t_valid = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    t_occ = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    imgs = [torch.zeros((h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    b = H.PtGatherBuffers(C.cast(ptr(t_sum), H._dp), C.cast(ptr(t_valid), H._u8p))
    rb = H.PtRaysBuffers(occluded=C.cast(ptr(t_occ), H._u8p))
    st = H.PtStats()

    def render(k):
        q = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), 2, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
        return lib.pt_render_device(cx, C.byref(cam), ptr(d_bg), C.byref(q), 0, ptr(imgs[k]), C.c_void_p(lib.pt_context_stream(cx, k)))
    rays = lambda: lib.pt_rays_device(cx, C.byref(rp), ptr(d_P), ptr(d_N), C.byref(rb), None)
    gather = lambda: lib.pt_gather_device(cx, C.byref(p), ptr(d_P), ptr(d_N), dp(bg3), C.byref(b), C.c_void_p(stream.cuda_stream))
    if overlapped:
        assert render(0) == H.OK and render(1) == H.OK and rays() == H.OK, lib.pt_last_error(cx)
        assert gather() == H.OK, lib.pt_last_error(cx)
        assert gather() == H.ERR_ARGUMENT  # one radiance / film / gather pass in flight per context ...
        hs, hv = np.full((n, 3), 9.0), np.full(n, 9, dtype=np.uint8)
        hb = H.PtGatherBuffers(dp(hs), hv.ctypes.data_as(H._u8p))
        assert lib.pt_gather(cx, C.byref(p), dp(P), dp(N), dp(bg3), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included,
        qp, rgb = H.PtRadianceParams(n, 0, 0, 7, 0, 0), np.full((n, 3), 9.0)
        assert lib.pt_radiance(cx, C.byref(qp), dp(P), dp(N), dp(bg3), dp(rgb), None) == H.ERR_ARGUMENT  # the radiance pass
        assert lib.pt_radiance_device(cx, C.byref(qp), ptr(d_P), ptr(d_N), ptr(d_bg), ptr(t_sum), None) == H.ERR_ARGUMENT
        fp = H.PtFilmParams(H.PtRect(0, 0, w - 1, h - 1), 1, 3, H.SAMPLE_RNG, 1)
        assert lib.pt_film_add(cx, film, C.byref(cam), dp(bg), C.byref(fp), None) == H.ERR_ARGUMENT  # and a film's add
        assert lib.pt_film_add_device(cx, film, C.byref(cam), ptr(d_bg), C.byref(fp), None) == H.ERR_ARGUMENT
        assert np.all(hs == 9.0) and np.all(hv == 9) and np.all(rgb == 9.0)
        ms = C.c_double(-1.0)
        assert lib.pt_gather_finish(cx, C.byref(ms)) == H.OK and ms.value > 0.0, lib.pt_last_error(cx)
        assert lib.pt_gather_finish(cx, None) == H.ERR_ARGUMENT and lib.pt_radiance_finish(cx, None) == H.ERR_ARGUMENT  # nothing in flight any more
        assert lib.pt_render_finish(cx, C.byref(st)) == H.OK and lib.pt_render_finish(cx, C.byref(st)) == H.OK and lib.pt_rays_finish(cx, None) == H.OK, lib.pt_last_error(cx)
    else:
        for k in (0, 1):
            assert render(k) == H.OK and lib.pt_render_finish(cx, C.byref(st)) == H.OK, lib.pt_last_error(cx)
        assert rays() == H.OK and lib.pt_rays_finish(cx, None) == H.OK, lib.pt_last_error(cx)
        assert gather() == H.OK and lib.pt_gather_finish(cx, None) == H.OK, lib.pt_last_error(cx)
    stream.synchronize(); torch.cuda.synchronize()
    results.append(dict(sum=t_sum.cpu().numpy().tobytes(), valid=t_valid.cpu().numpy().tobytes(), occ=t_occ.cpu().numpy().tobytes(),
                        img0=imgs[0].cpu().numpy().tobytes(), img1=imgs[1].cpu().numpy().tobytes()))
for k in results[0]:
    assert results[0][k] == results[1][k], k
assert results[1]["sum"] == ref["sum"].tobytes() and results[1]["valid"] == ref["valid"].tobytes()
assert any(results[1]["img0"]) and any(results[1]["img1"]) and 1 in results[1]["occ"] and 5 not in results[1]["occ"]
fp = H.PtFilmParams(H.PtRect(0, 0, w - 1, h - 1), 1, 3, H.SAMPLE_RNG, 1)
assert lib.pt_film_add(cx, film, C.byref(cam), dp(bg), C.byref(fp), None) == H.OK, lib.pt_last_error(cx)  # the pass is free again
assert lib.pt_film_destroy(cx, film) == H.OK
r.close()
assert (x * 2).sum().item() == 2048.0
print("gather into torch tensors ok")
""" % (root, root)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "gather into torch tensors ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


# ---- 9. refusals on a context
def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    c = case(host, H, "big-scene", "flat")
    ctx = c["r"].context
    n = 100
    P, N, bg = np.zeros((n, 3)), np.ones((n, 3)), np.array(BG)
    total, valid = np.full((n, 3), 3.0), np.full(n, 3, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ob = H.PtGatherBuffers(sum=dp(total), valid=valid.ctypes.data_as(H._u8p))
    ok = dict(n=n, samples=16, pass_index=0, seed=0, first_index=0, bias=0.0, flags=0)
    good = H.PtGatherParams(**ok)
    bad_eye = H.PtGatherParams(**dict(ok, flags=H.AO_FACE_EYE))
    bad_eye.eye[0] = float("nan")
    for fn in (lib.pt_gather, lib.pt_gather_device):
        assert fn(ctx, None, dp(P), dp(N), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(N), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), None, dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), None, C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), dp(bg), None, None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), dp(bg), C.byref(H.PtGatherBuffers()), None) == H.ERR_ARGUMENT
        for change in (dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=48), dict(samples=128), dict(bias=-1e-300), dict(bias=float("inf")),
                       dict(bias=float("nan")), dict(flags=2), dict(flags=0x80000001)):
            assert fn(ctx, C.byref(H.PtGatherParams(**dict(ok, **change))), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT, change
            assert lib.pt_last_error(ctx).startswith(b"pt_gather:"), change
        assert fn(ctx, C.byref(bad_eye), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(H.PtGatherParams(**dict(ok, n=0))), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(total == 3.0) and np.all(valid == 3)
    assert lib.pt_gather_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    nan_eye_unused = H.PtGatherParams(**ok)
    nan_eye_unused.eye[1] = float("nan")  # the eye is read with PT_AO_FACE_EYE only
    assert lib.pt_gather(ctx, C.byref(nan_eye_unused), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.OK
    assert np.all(valid == 1) and np.all(np.isfinite(total))
    bare = H.Context()
    assert lib.pt_gather(bare.handle, C.byref(good), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.ERR_NO_SCENE
    assert lib.pt_gather_device(bare.handle, C.byref(good), dp(P), dp(N), dp(bg), C.byref(ob), None) == H.ERR_NO_SCENE
    bare.close()
