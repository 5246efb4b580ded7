"""The probe pass (pt_probe / pt_probe_device / Renderer.probe / Renderer.probe_grid) on the GPU, bit for bit.

The yardstick is what exists: the numpy restatement of the probe contract (tests/probe_restate.py, equal to the host replay in every bit:
tests/test_probe_contract.py) makes each probe's rays and their nine basis values, Renderer.radiance - pinned to the oracle by tests/test_gpu_radiance.py -
shades the rays, flattened probe-major, with stream_base = first_index * S and sample = pass_index, and numpy weights and adds in the contract's order (per round
of 64 samples from zero in ascending k, the rounds left to right); invalid probes are zeros. `sh` and `valid` are compared exactly: there is no tolerance
anywhere in this file. The probes are what Renderer.aov finds under a 16 x 9 image, lifted 0.25 along the normal into free space, at most 24 per scene. The
background is not black, so a ray that leaves the scene shows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from probe_restate import project, restate  # noqa: E402
from scene_dsl import ASSETS  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 16, 9
MOST = 24
SEED = 7
BG = (0.25, 0.5, 1.0)
TRAVERSALS = ("flat", "hier", "kd")
SCENES = ("big-scene", "macho-cows", "soft-shadows", "glossy-reflection", "transmission-refraction")
WANT = ("sh", "valid")


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


def lifted(r, cam):
    """At most MOST of the points under a W x HT image, evenly taken, each lifted 0.25 along its normal"""
    aov = r.aov(cam, W, HT, want=("position", "normal", "node"))
    hit = np.flatnonzero(aov["node"].ravel() >= 0)
    assert len(hit) >= 8
    take = hit[np.linspace(0, len(hit) - 1, min(MOST, len(hit))).astype(int)]
    return np.ascontiguousarray(aov["position"].reshape(-1, 3)[take] + 0.25 * aov["normal"].reshape(-1, 3)[take])


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def close_renderers():
    yield
    for c in _CASES.values():
        c["r"].close()
    _CASES.clear()


def case(host, H, which, mname):
    """A renderer of the scene in one traversal and its probes: made once, shared, never written to."""
    key = (which, mname)
    if key not in _CASES:
        sc = host.Scene.example(which, assets=ASSETS)
        r = host.Renderer(sc, traversal(H, mname), kd_depth=10)
        P = lifted(r, sc.camera)
        P.setflags(write=False)
        _CASES[key] = dict(sc=sc, r=r, P=P, refs={})
    return _CASES[key]


def reference(r, P, S, seed=SEED, pas=0, first=0, bg=BG):
    """What the contract says, from the existing pass: (sh f64 (n, 9, 3), valid u8 (n,), the all-background answer (n, 9, 3))."""
    O, D, Y, valid = restate(P, S, seed, pas, first)
    n = len(P)
    if n == 0:
        return np.zeros((0, 9, 3)), valid, np.zeros((0, 9, 3))
    with np.errstate(over="ignore"):
        base = int(np.uint64(first) * np.uint64(S))  # (modulo 2^64, as the stream index is)
    rgb = r.radiance(np.ascontiguousarray(O.reshape(-1, 3)), np.ascontiguousarray(D.reshape(-1, 3)), bg, seed=seed, sample=pas, stream_base=base)["rgb"].reshape(n, S, 3)
    return project(Y, rgb, valid), valid, project(Y, np.broadcast_to(np.array(bg), rgb.shape), valid)


def case_reference(c, S, pas=0, seed=SEED, first=0):
    key = (S, pas, seed, first)
    if key not in c["refs"]:
        ref = reference(c["r"], c["P"], S, seed=seed, pas=pas, first=first)
        for a in ref:
            a.setflags(write=False)
        c["refs"][key] = ref
    return c["refs"][key]


def check(tag, got, ref):
    sh, valid = ref[0], ref[1]
    assert got["sh"].dtype == np.float64 and got["valid"].dtype == np.uint8 and got["sh"].shape == sh.shape
    assert np.array_equal(got["valid"], valid), f"{tag}: valid"
    bad = np.flatnonzero((bits(got["sh"]) != bits(sh)).reshape(len(sh), -1).any(axis=1))
    assert not len(bad), f"{tag}: sh differs at {len(bad)} of {len(sh)} probes, first {bad[:3]}: {got['sh'][bad[:1]]} != {sh[bad[:1]]}"


def shaded(ref):
    """(valid probes whose sh is not the all-background answer, valid probes)"""
    sh, valid, sky = ref
    return int(((bits(sh) != bits(sky)).reshape(len(sh), -1).any(axis=1) & (valid == 1)).sum()), int(valid.sum())


# ---- 1. parity with the radiance pass: every scene, every traversal, the direct write and the smallest fold
@pytest.mark.parametrize("mname", TRAVERSALS)
@pytest.mark.parametrize("which", SCENES)
def test_sh_and_valid_equal_the_radiance_pass_on_the_restated_rays(host, H, which, mname):
    c = case(host, H, which, mname)
    for S in (64, 128):
        ref = case_reference(c, S)
        some, valid = shaded(ref)
        print(f"{which} {mname} S={S}: {valid} valid probes of {len(c['P'])}, {some} with an sh other than the all-background answer")
        assert valid == len(c["P"]) and 10 * some >= valid and np.all(np.isfinite(ref[0])), "the guard is on the REFERENCE"
        got = c["r"].probe(c["P"], BG, samples=S, seed=SEED, want=WANT)
        check(f"{which} {mname} S={S}", got, ref)
        assert np.array_equal(bits(got["coeffs"]), bits(ref[0] * (4.0 * np.pi / S))) and got["kernel_ms"] > 0.0


@pytest.mark.parametrize("mname", TRAVERSALS)
def test_sixteen_rounds(host, H, mname):
    c = case(host, H, "big-scene", mname)
    ref = case_reference(c, 1024)
    assert shaded(ref)[0] > 0
    check(f"big-scene {mname} S=1024", c["r"].probe(c["P"], BG, samples=1024, seed=SEED, want=WANT), ref)
    assert not np.array_equal(bits(ref[0]), bits(case_reference(c, 128)[0]))


# ---- 2. how a batch is cut
def test_batch_sizes_cuts_and_an_empty_batch(host, H):
    c = case(host, H, "big-scene", "flat")
    r, P = c["r"], c["P"]
    run = lambda P, **kw: r.probe(P, BG, seed=SEED, want=WANT, **kw)
    for S in (64, 128):
        whole = reference(r, P[:5], S, first=5000)
        check(f"5 probes S={S}", run(P[:5].copy(), samples=S, first_index=5000), whole)
        for n in (1, 2, 3):
            check(f"n={n} S={S}", run(P[:n].copy(), samples=S, first_index=5000), tuple(a[:n] for a in whole))
        a, b = run(P[:2].copy(), samples=S, first_index=5000), run(P[2:5].copy(), samples=S, first_index=5002)
        check(f"cut at 2 of 5, S={S}", {k: np.concatenate([a[k], b[k]]) for k in WANT}, whole)
        shifted = run(P[2:5].copy(), samples=S, first_index=5000)
        assert not np.array_equal(bits(shifted["sh"]), bits(whole[0][2:5])), "first_index is part of the stream"
    empty = r.probe(np.zeros((0, 3)), BG, samples=128, want=WANT)
    assert empty["sh"].shape == (0, 9, 3) and empty["coeffs"].shape == (0, 9, 3) and empty["valid"].shape == (0,) and empty["kernel_ms"] == 0.0
    only = r.probe(P, BG, samples=128, seed=SEED, want=("valid",))  # one buffer alone
    assert sorted(only) == ["kernel_ms", "valid"] and np.all(only["valid"] == 1)
    big = 1 << 60  # the 64-bit stream product: (first_index + i) * S is reduced modulo 2^64 only, as stream_base + i is
    for S in (64, 1024):
        check(f"first_index 2^60 S={S}", run(P[:3].copy(), samples=S, first_index=big), reference(r, P[:3], S, first=big))


def test_a_call_across_the_scratch_bound_has_the_single_launchs_bits(monkeypatch, host, H):
    """PORTRAYER_PROBE_SCRATCH lowers the 32 MiB bound on the partial sums: at 1,000 bytes and S = 128 (432 bytes per probe) a launch holds two probes, so five
    take three launches and three folds inside one pass."""
    c = case(host, H, "macho-cows", "flat")
    P = c["P"][:5].copy()
    ref = reference(c["r"], P, 128, first=3)
    single = c["r"].probe(P, BG, samples=128, seed=SEED, first_index=3, want=WANT)
    check("one launch", single, ref)
    for bound in ("1000", "432", "1"):  # two probes per launch; one; the floor of one
        monkeypatch.setenv("PORTRAYER_PROBE_SCRATCH", bound)
        cut = c["r"].probe(P, BG, samples=128, seed=SEED, first_index=3, want=WANT)
        check(f"bound {bound}", cut, ref)
        assert cut["sh"].tobytes() == single["sh"].tobytes() and cut["kernel_ms"] > 0.0
    check("S = 64 keeps no partials", c["r"].probe(P, BG, samples=64, seed=SEED, first_index=3, want=WANT), reference(c["r"], P, 64, first=3))


# ---- 3. passes and seeds
def test_two_passes_differ_and_each_equals_its_reference(host, H):
    c = case(host, H, "macho-cows", "flat")
    refs = [case_reference(c, 128, pas=p) for p in (0, 1)]
    assert not np.array_equal(bits(refs[0][0]), bits(refs[1][0]))
    for p in (0, 1):
        check(f"pass {p}", c["r"].probe(c["P"], BG, samples=128, seed=SEED, pass_index=p, want=WANT), refs[p])


def test_the_seed_reaches_the_area_lights_draws(host, H):
    c = case(host, H, "soft-shadows", "flat")
    a, b = case_reference(c, 64), case_reference(c, 64, seed=SEED + 1)
    assert not np.array_equal(bits(a[0]), bits(b[0]))
    check("seed + 1", c["r"].probe(c["P"], BG, samples=64, seed=SEED + 1, want=WANT), b)


# ---- 4. invalid probes between valid ones
@pytest.mark.parametrize("which,mname,S", [("macho-cows", "flat", 64), ("big-scene", "kd", 128), ("transmission-refraction", "hier", 128)])
def test_invalid_probes_report_zeros_and_change_no_neighbour(host, H, which, mname, S):
    c = case(host, H, which, mname)
    ref = case_reference(c, S)
    P = c["P"].copy()
    spoil = np.array([1, 4, 5, 9])
    P[1, 1], P[4, 0], P[5, 2], P[9, 0] = np.nan, np.inf, -np.inf, 2e18
    want = [a.copy() for a in ref[:2]]
    for a in want:
        a[spoil] = 0
    got = c["r"].probe(P, BG, samples=S, seed=SEED, want=WANT)
    check(f"{which} {mname} with invalid probes", got, want)
    assert not got["sh"][spoil].any() and not got["valid"][spoil].any() and want[0].any()
    nothing = c["r"].probe(np.full((3, 3), np.nan), BG, samples=S, want=WANT)  # wavefronts without a single ray
    assert not nothing["sh"].any() and not nothing["valid"].any()


# ---- 5. parked frames in HBM
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_without_parked_frames_in_lds_the_bits_are_the_same(monkeypatch, host, H, mname):
    c = case(host, H, "transmission-refraction", mname)
    ref = case_reference(c, 128)  # (made with the default: frames parked in LDS)
    monkeypatch.setenv("PORTRAYER_PARK", "0")
    check(f"PORTRAYER_PARK=0 {mname}", c["r"].probe(c["P"], BG, samples=128, seed=SEED, want=WANT), ref)


# ---- 6. a moved scene
@pytest.mark.parametrize("mname", TRAVERSALS)
def test_after_an_update_the_pass_answers_for_the_moved_scene(host, H, mname):
    from test_gpu_update import grid
    scene_a, _, _ = grid(40, 0.0)()
    scene_b, cam_b, _ = grid(40, 0.7)()
    ha, hb, cam = host_glue.host_scene(scene_a), host_glue.host_scene(scene_b), host_glue.cam10(cam_b)
    r = host.Renderer(ha, traversal(H, mname), kd_depth=8)
    fresh = host.Renderer(hb, traversal(H, mname), kd_depth=8)
    P = lifted(fresh, cam)
    before = r.probe(P, BG, samples=128, seed=SEED, want=WANT)
    r.update(hb)
    moved, want = r.probe(P, BG, samples=128, seed=SEED, want=WANT), fresh.probe(P, BG, samples=128, seed=SEED, want=WANT)
    for k in WANT:
        assert moved[k].tobytes() == want[k].tobytes(), k
    ref = reference(fresh, P, 128)
    check(f"moved grid {mname}", want, ref)
    assert shaded(ref)[0] > 0 and before["sh"].tobytes() != want["sh"].tobytes()
    r.close()
    fresh.close()


# ---- 7. the grid form
def test_probe_grid_equals_probe_on_its_points(host, H):
    c = case(host, H, "big-scene", "flat")
    lo, hi = c["P"].min(axis=0), c["P"].max(axis=0)
    g = c["r"].probe_grid(lo, hi, (2, 3, 2), BG, samples=64, seed=SEED, first_index=9, want=WANT)
    assert g["points"].shape == (2, 3, 2, 3) and g["sh"].shape == (2, 3, 2, 9, 3) and g["coeffs"].shape == (2, 3, 2, 9, 3) and g["valid"].shape == (2, 3, 2)
    assert np.array_equal(g["points"][0, 0, 0], lo) and np.array_equal(g["points"][1, 2, 1], hi) and np.array_equal(g["points"][0, 1, 1], [lo[0], lo[1] + (hi[1] - lo[1]) * 0.5, hi[2]])
    flat = c["r"].probe(g["points"].reshape(-1, 3), BG, samples=64, seed=SEED, first_index=9, want=WANT)
    assert g["sh"].tobytes() == flat["sh"].tobytes() and g["valid"].tobytes() == flat["valid"].tobytes() and g["coeffs"].tobytes() == flat["coeffs"].tobytes()
    check("the grid's points", flat, reference(c["r"], g["points"].reshape(-1, 3), 64, first=9))


# ---- 8. device buffers, and the pass among the others
def test_device_tensors_on_a_torch_stream_and_the_passes_refused_meanwhile(H):
    """pt_probe_device with positions and results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first.
    While it is open a second radiance, film, gather or probe pass is refused."""
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
aov = r.aov(sc.camera, 16, 9, want=("position", "normal", "node"))
hit = aov["node"].ravel() >= 0
P = np.ascontiguousarray((aov["position"].reshape(-1, 3) + 0.25 * aov["normal"].reshape(-1, 3))[hit][:24])
N = np.ascontiguousarray(aov["normal"].reshape(-1, 3)[hit][:24])
n = len(P)
bg3 = np.array([0.25, 0.5, 1.0])
w, h = 64, 32
cam = host.camera(sc.camera, w, h)
bg = default_background(w, h)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
d_P, d_N, d_bg = t(P), t(N), t(bg)
ptr = lambda tensor: C.c_void_p(tensor.data_ptr())
dp = lambda a: a.ctypes.data_as(H._dp)
film = C.c_void_p()
assert lib.pt_film_create(cx, w, h, C.byref(film)) == H.OK
for S in (64, 256):
    ref = r.probe(P, bg3, samples=S, seed=7, pass_index=2, first_index=11, want=("sh", "valid"))
    assert ref["valid"].sum() == n and ref["sh"].any()
    p = H.PtProbeParams(n, S, 2, 7, 11)
    t_sh = torch.full((n, 9, 3), 5.0, dtype=torch.float64, device=dev)
    t_valid = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    b = H.PtProbeBuffers(C.cast(ptr(t_sh), H._dp), C.cast(ptr(t_valid), H._u8p))
    probe = lambda: lib.pt_probe_device(cx, C.byref(p), ptr(d_P), dp(bg3), C.byref(b), C.c_void_p(stream.cuda_stream))
    assert probe() == H.OK, lib.pt_last_error(cx)
    assert probe() == H.ERR_ARGUMENT  # one radiance / film / gather / probe pass in flight per context ...
    hs, hv = np.full((n, 9, 3), 9.0), np.full(n, 9, dtype=np.uint8)
    hb = H.PtProbeBuffers(dp(hs), hv.ctypes.data_as(H._u8p))
    assert lib.pt_probe(cx, C.byref(p), dp(P), dp(bg3), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included,
    gs = np.full((n, 3), 9.0)
    gp, gb = H.PtGatherParams(n, 16, 0, 7, 0, 0.0, 0, (C.c_double * 3)(0.0, 0.0, 0.0)), H.PtGatherBuffers(dp(gs), None)
    assert lib.pt_gather(cx, C.byref(gp), dp(P), dp(N), dp(bg3), C.byref(gb), None) == H.ERR_ARGUMENT  # a gather pass,
    assert lib.pt_gather_device(cx, C.byref(gp), ptr(d_P), ptr(d_N), dp(bg3), C.byref(gb), None) == H.ERR_ARGUMENT
    qp, rgb = H.PtRadianceParams(n, 0, 0, 7, 0, 0), np.full((n, 3), 9.0)
    assert lib.pt_radiance(cx, C.byref(qp), dp(P), dp(N), dp(bg3), dp(rgb), None) == H.ERR_ARGUMENT  # the radiance pass
    assert lib.pt_radiance_device(cx, C.byref(qp), ptr(d_P), ptr(d_N), ptr(d_bg), ptr(t_sh), None) == H.ERR_ARGUMENT
    fp = H.PtFilmParams(H.PtRect(0, 0, w - 1, h - 1), 1, 3, H.SAMPLE_RNG, 1)
    assert lib.pt_film_add(cx, film, C.byref(cam), dp(bg), C.byref(fp), None) == H.ERR_ARGUMENT  # and a film's add
    assert lib.pt_film_add_device(cx, film, C.byref(cam), ptr(d_bg), C.byref(fp), None) == H.ERR_ARGUMENT
    assert np.all(hs == 9.0) and np.all(hv == 9) and np.all(rgb == 9.0) and np.all(gs == 9.0)
    ms = C.c_double(-1.0)
    assert lib.pt_probe_finish(cx, C.byref(ms)) == H.OK and ms.value > 0.0, lib.pt_last_error(cx)
    assert lib.pt_probe_finish(cx, None) == H.ERR_ARGUMENT and lib.pt_radiance_finish(cx, None) == H.ERR_ARGUMENT  # nothing in flight any more
    stream.synchronize(); torch.cuda.synchronize()
    assert t_sh.cpu().numpy().tobytes() == ref["sh"].tobytes() and t_valid.cpu().numpy().tobytes() == ref["valid"].tobytes(), S
fp = H.PtFilmParams(H.PtRect(0, 0, w - 1, h - 1), 1, 3, H.SAMPLE_RNG, 1)
assert lib.pt_film_add(cx, film, C.byref(cam), dp(bg), C.byref(fp), None) == H.OK, lib.pt_last_error(cx)  # the pass is free again
assert lib.pt_film_destroy(cx, film) == H.OK
r.close()
assert (x * 2).sum().item() == 2048.0
print("probe into torch tensors ok")
""" % (root, root)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0 and "probe into torch tensors ok" in done.stdout, done.stdout[-2000:] + done.stderr[-4000:]


# ---- 9. refusals on a context
def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    c = case(host, H, "big-scene", "flat")
    ctx = c["r"].context
    n = 10
    P, bg = np.zeros((n, 3)), np.array(BG)
    sh, valid = np.full((n, 9, 3), 3.0), np.full(n, 3, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    ob = H.PtProbeBuffers(sh=dp(sh), valid=valid.ctypes.data_as(H._u8p))
    ok = dict(n=n, samples=64, pass_index=0, seed=0, first_index=0)
    good = H.PtProbeParams(**ok)
    for fn in (lib.pt_probe, lib.pt_probe_device):
        assert fn(ctx, None, dp(P), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), None, C.byref(ob), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(bg), None, None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(P), dp(bg), C.byref(H.PtProbeBuffers()), None) == H.ERR_ARGUMENT
        for change in (dict(n=H.PROBE_MAX + 1), dict(samples=0), dict(samples=32), dict(samples=96), dict(samples=2048), dict(samples=65)):
            assert fn(ctx, C.byref(H.PtProbeParams(**dict(ok, **change))), dp(P), dp(bg), C.byref(ob), None) == H.ERR_ARGUMENT, change
            assert lib.pt_last_error(ctx).startswith(b"pt_probe:"), change
        assert fn(ctx, C.byref(H.PtProbeParams(**dict(ok, n=0))), dp(P), dp(bg), C.byref(ob), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(sh == 3.0) and np.all(valid == 3)
    assert lib.pt_probe_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    assert lib.pt_probe(ctx, C.byref(good), dp(P), dp(bg), C.byref(ob), None) == H.OK
    assert np.all(valid == 1) and np.all(np.isfinite(sh))
    bare = H.Context()
    assert lib.pt_probe(bare.handle, C.byref(good), dp(P), dp(bg), C.byref(ob), None) == H.ERR_NO_SCENE
    assert lib.pt_probe_device(bare.handle, C.byref(good), dp(P), dp(bg), C.byref(ob), None) == H.ERR_NO_SCENE
    bare.close()
