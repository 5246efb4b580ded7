"""The ambient-occlusion pass (pt_ao / pt_ao_device / Renderer.ao / Renderer.ao_camera) on the GPU, bit for bit.

The yardstick is the pass that exists: the numpy restatement of the contract (tests/test_ao_contract.py, equal to the host replay in every bit) makes each point's
rays, Renderer.rays(o, d, any_hit=True, t_max=radius) - pinned to the oracle by tests/test_gpu_segments.py - answers them, numpy counts and sums left to right.
Counts, `valid` and `bent` are compared exactly, in both work layouts of the kernel. The points are what Renderer.aov finds under a 67 x 37 image (2,479 points,
misses included: they are invalid points), the normals turned towards the camera's eye."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402
from test_ao_contract import restate  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37
NPTS = W * HT
SEED = 7
LAYOUTS = ("point", "sample")
TRAVERSALS = ("flat", "hier", "kd")
RADIUS = {"primitives-simple": 2.0, "big-scene": np.inf, "macho-cows": np.inf, "robot-alarm-clock": np.inf}
WANT = ("occluded", "valid", "bent")


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


def reference(r, P, N, S, radius, seed=SEED, pas=0, first=0, bias=0.0, eye=None):
    """What the contract says, from the existing pass: (occluded u32, valid u8, bent f64, the per-ray flags)."""
    O, D, valid = restate(P, N, S, seed, pas, first, bias, eye)
    n = len(P)
    if n == 0:
        return np.zeros(0, dtype=np.uint32), valid, np.zeros((0, 3)), np.zeros((0, S), dtype=np.uint8)
    occ = r.rays(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), any_hit=True, t_max=float(radius))["occluded"].reshape(n, S)
    bent = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for k in range(S):  # ascending k, left to right, from (0, 0, 0)
            bent = np.where((occ[:, k] == 0)[:, None], bent + D[:, k, :], bent)
    bent[valid == 0] = 0.0
    return occ.sum(axis=1).astype(np.uint32), valid, bent, occ


def case_reference(c, S, radius, pas=0, bias=0.0):
    key = (S, float(radius), pas, bias)
    if key not in c["refs"]:
        ref = reference(c["r"], c["P"], c["N"], S, radius, pas=pas, bias=bias, eye=c["eye"])
        for a in ref:
            a.setflags(write=False)
        c["refs"][key] = ref
    return c["refs"][key]


def run(monkeypatch, r, layout, P, N, **kw):
    monkeypatch.setenv("PORTRAYER_AO_LAYOUT", layout)
    return r.ao(P, N, want=WANT, **kw)


def check(tag, got, ref):
    occ, valid, bent, _ = ref
    assert got["occluded"].dtype == np.uint32 and got["valid"].dtype == np.uint8 and got["bent"].dtype == np.float64
    assert np.array_equal(got["valid"], valid), f"{tag}: valid"
    bad = np.flatnonzero(got["occluded"] != occ)
    assert not len(bad), f"{tag}: occluded differs at {len(bad)} points, first {bad[:5]}: {got['occluded'][bad[:5]]} != {occ[bad[:5]]}"
    assert np.array_equal(bits(got["bent"]), bits(bent)), f"{tag}: bent"


def partial(ref, S):
    occ, valid = ref[0], ref[1]
    return int(((occ > 0) & (occ < S) & (valid == 1)).sum()), int(valid.sum())


# ---- 1. parity with the existing pass: every scene, every traversal, both layouts
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", list(RADIUS))
def test_counts_valid_and_bent_equal_the_ray_queries_on_the_restated_rays(monkeypatch, host, H, which, mname):
    c = case(host, H, which, mname)
    radius = RADIUS[which]
    ref = case_reference(c, 16, radius)
    some, valid = partial(ref, 16)
    print(f"{which} {mname}: {valid} valid points of {NPTS}, {some} with 0 < occluded < 16, mean occluded {ref[0][ref[1] == 1].mean():.2f}")
    assert np.array_equal(ref[1], c["hit"].astype(np.uint8)), "aov's misses are the invalid points"
    if which != "robot-alarm-clock":  # (the three scenes whose counts were taken from the CPU oracle before any of this ran)
        assert 4 * some >= valid > 1000, "a pass that answers all zeros - or all S - must not pass"
    assert some > 0
    for layout in LAYOUTS:
        got = run(monkeypatch, c["r"], layout, c["P"], c["N"], samples=16, radius=radius, seed=SEED, eye=c["eye"])
        check(f"{which} {mname} {layout}", got, ref)
        assert np.array_equal(bits(got["visibility"]), bits(1.0 - ref[0] / 16.0)) and np.all(got["visibility"][ref[1] == 0] == 1.0)
    if np.isinf(radius):  # the unbounded limit is pt_rays
        O, D, _ = restate(c["P"], c["N"], 16, SEED, 0, 0, 0.0, c["eye"])
        occ = c["r"].rays(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), any_hit=True)["occluded"].reshape(-1, 16)
        assert np.array_equal(occ, ref[3])


@pytest.mark.parametrize("mname", TRAVERSALS)
def test_other_radii_sample_counts_and_a_bias(monkeypatch, host, H, mname):
    c = case(host, H, "primitives-simple", mname)
    for S, radius, bias in ((16, 0.5, 0.0), (1, 2.0, 0.0), (4, 2.0, 0.0), (64, 2.0, 0.0), (8, 2.0, 0.015625)):
        ref = case_reference(c, S, radius, bias=bias)
        print(f"primitives-simple {mname} S={S} radius={radius} bias={bias}: partial / valid = {partial(ref, S)}, occluded rays {int(ref[0].sum())}")
        assert 0 < ref[0].sum() < S * ref[1].sum()
        for layout in LAYOUTS:
            check(f"S={S} radius={radius} {layout}", run(monkeypatch, c["r"], layout, c["P"], c["N"], samples=S, radius=radius, bias=bias, seed=SEED, eye=c["eye"]), ref)
    near, far = case_reference(c, 16, 0.5), case_reference(c, 16, 2.0)
    assert np.all(near[0] <= far[0]) and near[0].sum() < far[0].sum(), "a larger radius only adds occluders"


# ---- 2. how a batch is cut
@pytest.mark.parametrize("layout", LAYOUTS)
def test_batch_sizes_cuts_and_an_empty_batch(monkeypatch, host, H, layout):
    c = case(host, H, "big-scene", "flat")
    r, P, N, eye = c["r"], c["P"], c["N"], c["eye"]
    start = int(np.flatnonzero(c["hit"])[0])  # (the image's first rows see the sky: start where the points are)
    whole = reference(r, P, N, 16, np.inf, first=5000, eye=eye)
    check("2,479 points", run(monkeypatch, r, layout, P, N, samples=16, seed=SEED, first_index=5000, eye=eye), whole)
    for n in (1, 3, 63, 65):
        got = run(monkeypatch, r, layout, P[start:start + n].copy(), N[start:start + n].copy(), samples=16, seed=SEED, first_index=5000 + start, eye=eye)
        check(f"n={n}", got, tuple(a[start:start + n] for a in whole))
    for S in (1, 4, 64):  # a partial last wavefront at every group size
        ref = reference(r, P[start:start + 65], N[start:start + 65], S, np.inf, first=start, eye=eye)
        check(f"n=65 S={S}", run(monkeypatch, r, layout, P[start:start + 65].copy(), N[start:start + 65].copy(), samples=S, seed=SEED, first_index=start, eye=eye), ref)
    a = run(monkeypatch, r, layout, P[:1000].copy(), N[:1000].copy(), samples=16, seed=SEED, first_index=5000, eye=eye)
    b = run(monkeypatch, r, layout, P[1000:].copy(), N[1000:].copy(), samples=16, seed=SEED, first_index=6000, eye=eye)
    check("cut at 1,000", {k: np.concatenate([a[k], b[k]]) for k in WANT}, whole)
    shifted = run(monkeypatch, r, layout, P[1000:].copy(), N[1000:].copy(), samples=16, seed=SEED, first_index=5000, eye=eye)
    assert not np.array_equal(shifted["occluded"], whole[0][1000:]), "first_index is part of the stream"
    empty = run(monkeypatch, r, layout, np.zeros((0, 3)), np.zeros((0, 3)), samples=16)
    assert empty["occluded"].shape == (0,) and empty["bent"].shape == (0, 3) and empty["visibility"].shape == (0,) and empty["kernel_ms"] == 0.0
    only = r.ao(P, N, samples=16, seed=SEED, first_index=5000, eye=eye, want=("bent",))  # one buffer alone
    assert sorted(only) == ["bent", "kernel_ms"] and np.array_equal(bits(only["bent"]), bits(whole[2]))


def test_passes_differ_and_each_matches_its_restatement(monkeypatch, host, H):
    c = case(host, H, "macho-cows", "flat")
    refs = [case_reference(c, 16, np.inf, pas=p) for p in (0, 1)]
    assert not np.array_equal(refs[0][0], refs[1][0]) and not np.array_equal(bits(refs[0][2]), bits(refs[1][2]))
    for p in (0, 1):
        for layout in LAYOUTS:
            check(f"pass {p} {layout}", run(monkeypatch, c["r"], layout, c["P"], c["N"], samples=16, seed=SEED, pass_index=p, eye=c["eye"]), refs[p])
    other_seed = c["r"].ao(c["P"], c["N"], samples=16, seed=SEED + 1, eye=c["eye"])["occluded"]
    assert not np.array_equal(other_seed, refs[0][0])


# ---- 3. invalid points inside wavefronts
@pytest.mark.parametrize("which,mname", [("macho-cows", "flat"), ("big-scene", "kd"), ("robot-alarm-clock", "hier")])
def test_invalid_points_report_zeros_and_change_no_neighbour(monkeypatch, host, H, which, mname):
    c = case(host, H, which, mname)
    ref = case_reference(c, 16, RADIUS[which])
    P, N = c["P"].copy(), c["N"].copy()
    rng = np.random.default_rng(5)
    hit = np.flatnonzero(c["hit"])
    spoil = rng.choice(hit, size=len(hit) // 5, replace=False)  # scattered: nearly every wavefront of either layout holds some
    kind = np.arange(len(spoil)) % 5
    P[spoil[kind == 0], 1] = np.nan
    N[spoil[kind == 1]] = 0.0
    N[spoil[kind == 2], 2] = -np.inf
    P[spoil[kind == 3], 0] = 2e18
    P[spoil[kind == 4]], N[spoil[kind == 4]] = 0.0, 0.0  # what aov writes where nothing is hit
    want = [a.copy() for a in ref[:3]]
    for a in want:
        a[spoil] = 0
    for layout in LAYOUTS:
        got = run(monkeypatch, c["r"], layout, P, N, samples=16, radius=RADIUS[which], seed=SEED, eye=c["eye"])
        check(f"{which} {mname} {layout} with invalid points", got, (want[0], want[1], want[2], None))
        assert not got["occluded"][spoil].any() and not got["valid"][spoil].any() and not got["bent"][spoil].any() and np.all(got["visibility"][spoil] == 1.0)
    assert want[0].sum() > 0
    nothing = c["r"].ao(np.full((130, 3), np.nan), np.ones((130, 3)), samples=4, want=WANT)  # wavefronts without a single ray
    assert not nothing["occluded"].any() and not nothing["valid"].any() and not nothing["bent"].any()


# ---- 4. the camera form
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", ["big-scene", "macho-cows"])
def test_ao_camera_equals_ao_fed_with_the_aov_arrays(monkeypatch, host, H, which, mname):
    c = case(host, H, which, mname)
    ref = case_reference(c, 16, RADIUS[which])
    turned = int((((c["N"] * (c["P"] - c["eye"])).sum(axis=1) > 0.0) & c["hit"]).sum())
    print(f"{which} {mname}: {turned} first hits face away from the eye")
    if which == "big-scene":
        assert turned > 0, "PT_AO_FACE_EYE must have something to turn"
    for layout in LAYOUTS:
        monkeypatch.setenv("PORTRAYER_AO_LAYOUT", layout)
        got = c["r"].ao_camera(c["sc"].camera, W, HT, samples=16, radius=RADIUS[which], seed=SEED, want=WANT)
        assert got["occluded"].shape == (HT, W) and got["valid"].shape == (HT, W) and got["bent"].shape == (HT, W, 3) and got["visibility"].shape == (HT, W)
        check(f"{which} {mname} {layout} ao_camera", {k: got[k].reshape((NPTS,) + got[k].shape[2:]) for k in WANT}, ref)
        assert got["kernel_ms"] > 0.0
    smaller = c["r"].ao_camera(c["sc"].camera, 16, 8, samples=4, want=("occluded",))  # the renderer's scratch serves a smaller image after a larger one
    P8 = c["r"].aov(c["sc"].camera, 16, 8, want=("position", "normal"))
    eye8 = np.array(list(host.camera(c["sc"].camera, 16, 8).eye))
    assert np.array_equal(smaller["occluded"].ravel(), c["r"].ao(P8["position"].reshape(-1, 3), P8["normal"].reshape(-1, 3), samples=4, eye=eye8)["occluded"])


# ---- 5. device buffers, and the pass among the others
def test_device_tensors_on_a_torch_stream_equal_the_host_path(H):
    """pt_ao_device with points and results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first;
    while it is open no second ray-query pass of any kind is accepted, and pt_ao_finish closes it."""
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
from scene_dsl import ASSETS
lib = H.lib()
sc = host.Scene.example("macho-cows", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
aov = r.aov(sc.camera, 67, 37, want=("position", "normal"))
P, N = np.ascontiguousarray(aov["position"].reshape(-1, 3)), np.ascontiguousarray(aov["normal"].reshape(-1, 3))
n = len(P)
eye = list(host.camera(sc.camera, 67, 37).eye)
for layout in ("point", "sample"):
    os.environ["PORTRAYER_AO_LAYOUT"] = layout
    ref = r.ao(P, N, samples=16, radius=3.0, seed=7, pass_index=2, first_index=11, eye=eye, want=("occluded", "valid", "bent"))
    assert 0 < ref["occluded"].sum() < 16 * ref["valid"].sum()
    d_P, d_N = torch.from_numpy(P).to(dev), torch.from_numpy(N).to(dev)
    t_occ = torch.full((n,), 5, dtype=torch.int32, device=dev)
    t_valid = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    t_bent = torch.full((n, 3), 5.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    b = H.PtAoBuffers(C.cast(C.c_void_p(t_occ.data_ptr()), H._up), C.cast(C.c_void_p(t_valid.data_ptr()), H._u8p), C.cast(C.c_void_p(t_bent.data_ptr()), H._dp))
    p = H.PtAoParams(n, 16, 2, 7, 11, 3.0, 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*eye))
    args = (r.context, C.byref(p), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.byref(b), C.c_void_p(stream.cuda_stream))
    assert lib.pt_ao_device(*args) == H.OK, lib.pt_last_error(r.context)
    assert lib.pt_ao_device(*args) == H.ERR_ARGUMENT  # one ray-query pass in flight per context ...
    occ = np.full(n, 9, dtype=np.uint32)
    hb = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up))
    assert lib.pt_ao(r.context, C.byref(p), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included,
    rp, flags = H.PtRaysParams(n, 1, 0), np.full(n, 9, dtype=np.uint8)
    rb = H.PtRaysBuffers(occluded=flags.ctypes.data_as(H._u8p))
    assert lib.pt_rays(r.context, C.byref(rp), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(rb), None) == H.ERR_ARGUMENT  # and the ray queries'
    assert lib.pt_segments_device(r.context, C.byref(rp), C.c_void_p(d_P.data_ptr()), C.c_void_p(d_N.data_ptr()), C.c_void_p(d_P.data_ptr()), C.byref(rb), None) == H.ERR_ARGUMENT
    assert np.all(occ == 9) and np.all(flags == 9)
    ms = C.c_double(-1.0)
    assert lib.pt_ao_finish(r.context, C.byref(ms)) == H.OK and ms.value > 0.0
    assert lib.pt_ao_finish(r.context, None) == H.ERR_ARGUMENT and lib.pt_rays_finish(r.context, None) == H.ERR_ARGUMENT  # nothing in flight any more
    stream.synchronize()
    assert t_occ.cpu().numpy().view(np.uint32).tobytes() == ref["occluded"].tobytes(), layout
    assert t_valid.cpu().numpy().tobytes() == ref["valid"].tobytes() and t_bent.cpu().numpy().tobytes() == ref["bent"].tobytes(), layout
    assert lib.pt_rays(r.context, C.byref(rp), P.ctypes.data_as(H._dp), N.ctypes.data_as(H._dp), C.byref(rb), None) == H.OK  # the pass is free again
r.close()
assert (x * 2).sum().item() == 2048.0
print("ao into torch tensors ok")
""" % (root, root)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "ao into torch tensors ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


def test_a_render_and_an_aov_pass_in_flight_around_an_ao_pass(H, host):
    """pt_render_device on both slots and a pt_aov_device pass in flight, then pt_ao_device on a stream: every result equals what the same calls give one after
    the other on a second context."""
    import device_glue
    from example_scenes import EXAMPLES
    w, h, samples = 160, 96, 2
    bg = default_background(w, h)
    scene, cam0, _ = EXAMPLES["macho-cows"]()
    c = case(host, H, "macho-cows", "flat")
    P, N, n = c["P"], c["N"], NPTS
    lib = H.lib()
    camera = device_glue.camera_struct(cam0, w, h)
    results = []
    for overlapped in (False, True):
        ds = device_glue.DeviceScene(scene, H.TRAVERSE_FLAT)
        ctx = H.Context()
        ds.upload(ctx)
        cx = ctx.handle

        def dev(arr=None, nbytes=0):
            ptr = C.c_void_p()
            assert lib.pt_device_alloc(cx, arr.nbytes if arr is not None else nbytes, C.byref(ptr)) == 0
            if arr is not None:
                assert lib.pt_copy_to_device(cx, ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes) == 0
            return ptr
        d_bg, d_P, d_N = dev(bg), dev(P), dev(N)
        d_img, d_img2, d_depth, d_occ, d_bent = dev(nbytes=w * h * 3), dev(nbytes=w * h * 3), dev(nbytes=w * h * 8), dev(nbytes=n * 4), dev(nbytes=n * 24)
        st = H.PtStats()
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp))
        op = H.PtAoParams(n, 16, 0, SEED, 0, float("inf"), 0.0, H.AO_FACE_EYE, (C.c_double * 3)(*c["eye"]))
        ob = H.PtAoBuffers(occluded=C.cast(d_occ, H._up), bent=C.cast(d_bent, H._dp))

        def render(k, img):
            rp = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            return lib.pt_render_device(cx, C.byref(camera), d_bg, C.byref(rp), 0, img, C.c_void_p(lib.pt_context_stream(cx, k)))
        ao = lambda: lib.pt_ao_device(cx, C.byref(op), d_P, d_N, C.byref(ob), C.c_void_p(lib.pt_context_stream(cx, 0)))
        if overlapped:
            assert render(0, d_img) == 0 and render(1, d_img2) == 0 and lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0, lib.pt_last_error(cx)
            assert ao() == 0, lib.pt_last_error(cx)
            assert ao() == H.ERR_ARGUMENT
            assert lib.pt_ao_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
        else:
            for k, img in ((0, d_img), (1, d_img2)):
                assert render(k, img) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0, lib.pt_last_error(cx)
            assert lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert ao() == 0 and lib.pt_ao_finish(cx, None) == 0, lib.pt_last_error(cx)
        out = {}
        for name, ptr, arr in (("img", d_img, np.zeros((h, w, 3), dtype=np.uint8)), ("img2", d_img2, np.zeros((h, w, 3), dtype=np.uint8)), ("depth", d_depth, np.zeros((h, w))),
                               ("occ", d_occ, np.zeros(n, dtype=np.uint32)), ("bent", d_bent, np.zeros((n, 3)))):
            assert lib.pt_copy_from_device(cx, arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
            out[name] = arr
        for ptr in (d_bg, d_P, d_N, d_img, d_img2, d_depth, d_occ, d_bent):
            lib.pt_device_free(cx, ptr)
        ctx.close()
        results.append(out)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), k
    got = results[1]
    ref = case_reference(c, 16, np.inf)
    assert got["img"].any() and got["img2"].any() and np.isfinite(got["depth"]).any()
    assert np.array_equal(got["occ"], ref[0]) and np.array_equal(bits(got["bent"]), bits(ref[2]))


# ---- 6. a moved scene
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_after_an_update_the_pass_answers_for_the_moved_scene(monkeypatch, host, H, mname):
    from test_gpu_update import grid
    scene_a, cam_a, _ = grid(40, 0.0)()
    scene_b, cam_b, _ = grid(40, 0.7)()
    ha, hb, cam = host_glue.host_scene(scene_a), host_glue.host_scene(scene_b), host_glue.cam10(cam_b)
    r = host.Renderer(ha, traversal(H, mname), kd_depth=8)
    before = r.ao_camera(cam, W, HT, samples=16, radius=1.5, seed=SEED, want=WANT)
    r.update(hb)
    fresh = host.Renderer(hb, traversal(H, mname), kd_depth=8)
    for layout in LAYOUTS:
        monkeypatch.setenv("PORTRAYER_AO_LAYOUT", layout)
        moved, want = r.ao_camera(cam, W, HT, samples=16, radius=1.5, seed=SEED, want=WANT), fresh.ao_camera(cam, W, HT, samples=16, radius=1.5, seed=SEED, want=WANT)
        for k in WANT:
            assert moved[k].tobytes() == want[k].tobytes(), (layout, k)
    aov = fresh.aov(cam, W, HT, want=("position", "normal"))
    eye = np.array(list(host.camera(cam, W, HT).eye))
    ref = reference(fresh, aov["position"].reshape(-1, 3), aov["normal"].reshape(-1, 3), 16, 1.5, eye=eye)
    check(f"moved grid {mname}", {k: want[k].reshape((NPTS,) + want[k].shape[2:]) for k in WANT}, ref)
    assert 0 < ref[0].sum() and not np.array_equal(before["occluded"], want["occluded"])
    r.close()
    fresh.close()


# ---- 7. refusals on a context
def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    c = case(host, H, "primitives-simple", "flat")
    ctx = c["r"].context
    n = 100
    P, N = np.zeros((n, 3)), np.ones((n, 3))
    occ, bent = np.full(n, 3, dtype=np.uint32), np.full((n, 3), 3.0)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ob = H.PtAoBuffers(occluded=occ.ctypes.data_as(H._up), bent=dp(bent))
    ok = dict(n=n, samples=16, pass_index=0, seed=0, first_index=0, radius=1.0, bias=0.0, flags=0)
    good = H.PtAoParams(**ok)
    bad_eye = H.PtAoParams(**dict(ok, flags=H.AO_FACE_EYE))
    bad_eye.eye[0] = float("nan")
    for fn in (lib.pt_ao, lib.pt_ao_device):
        assert fn(ctx, None, dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), None, C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), None, None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(N), C.byref(H.PtAoBuffers()), None) == H.ERR_ARGUMENT
        for change in (dict(n=H.AO_MAX + 1), dict(samples=0), dict(samples=3), dict(samples=48), dict(samples=128), dict(radius=float("nan")), dict(radius=1e-5), dict(radius=0.0),
                       dict(radius=-2.0), dict(bias=-1e-300), dict(bias=float("inf")), dict(bias=float("nan")), dict(flags=2), dict(flags=0x80000001)):
            assert fn(ctx, C.byref(H.PtAoParams(**dict(ok, **change))), dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT, change
            assert lib.pt_last_error(ctx).startswith(b"pt_ao:"), change
        assert fn(ctx, C.byref(bad_eye), dp(P), dp(N), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(H.PtAoParams(**dict(ok, n=0))), dp(P), dp(N), C.byref(ob), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(occ == 3) and np.all(bent == 3.0)
    assert lib.pt_ao_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    nan_eye_unused = H.PtAoParams(**ok)
    nan_eye_unused.eye[1] = float("nan")  # the eye is read with PT_AO_FACE_EYE only
    assert lib.pt_ao(ctx, C.byref(nan_eye_unused), dp(P), dp(N), C.byref(ob), None) == H.OK
    assert lib.pt_ao(ctx, C.byref(H.PtAoParams(**dict(ok, radius=float("inf")))), dp(P), dp(N), C.byref(ob), None) == H.OK
    bare = H.Context()
    assert lib.pt_ao(bare.handle, C.byref(good), dp(P), dp(N), C.byref(ob), None) == H.ERR_NO_SCENE
    assert lib.pt_ao_device(bare.handle, C.byref(good), dp(P), dp(N), C.byref(ob), None) == H.ERR_NO_SCENE
    bare.close()
