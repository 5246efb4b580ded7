"""The ray-query pass (pt_rays / pt_rays_device / Renderer.rays) against the oracle's po_cast_rays, bit for bit.

Every comparison in this file is exact: bits() equality for f64, array equality for integers. No ray is left out of a comparison except the invalid rays
a test injects itself, whose number it knows and asserts. The batches are built to be what camera rays never were: origins inside and outside the scene
and ON its surfaces (hit points re-cast along the normal and along the reflected direction), direction lengths over [1e-3, 1e3], exactly axis-parallel
directions, -0 components - in seeded random order, so that nearly every wavefront mixes octants."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402
from test_gpu_aov import W, HT, bits, cast_one_ray, compare, first_use_order, modes, oracle_aov, packed_tri_off  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ("t", "position", "normal", "node", "sub", "material", "occluded")
N_RAYS = 100_000


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def oracle_rays(O, ps, o, d, mode, kd_depth, workers=16):
    """po_cast_rays over the batch, split over `workers` host threads: t, id, point and the world normal normalised as material.rs:123-125 does it
    (as test_gpu_aov.oracle_aov)."""
    parts = [p for p in np.array_split(np.arange(len(o)), workers) if len(p)]
    with ThreadPoolExecutor(max_workers=workers) as ex:
        res = list(ex.map(lambda p: O.cast_rays(ps, o[p], d[p], mode=mode, kd_depth=kd_depth), parts))
    t, ids, pt, nr = (np.concatenate([r[k] for r in res]) for k in range(4))
    hit = ids >= 0
    with np.errstate(all="ignore"):
        s = (nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]
        n = nr / np.sqrt(s)[:, None]
    n[~hit] = 0.0
    return dict(t=t, id=ids, point=pt, normal=n)


def as_aov(got):
    return dict(got, depth=got["t"])


def scene_box(flat):
    """A finite box around the flattened nodes' bounds (an unbounded primitive does not widen it beyond 1e3 per axis)."""
    b = np.nan_to_num(flat["bounds"], nan=0.0, posinf=1e3, neginf=-1e3)
    lo, hi = np.clip(b[:, :3].min(axis=0), -1e3, 1e3), np.clip(b[:, 3:].max(axis=0), -1e3, 1e3)
    return lo, np.maximum(hi, lo + 1e-3)


def unit_dirs(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def incoherent_batch(O, ps, flat, seed, n=N_RAYS):
    """About n rays as the module docstring describes them; the surface origins come from the oracle's (flat_scene) hits of the first batch."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(flat)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    n0 = (2 * n) // 5
    inside = c + e * rng.uniform(-1, 1, size=(n0 // 2, 3))
    shell = unit_dirs(rng, n0 - n0 // 2) * rng.uniform(1.2, 4.0, size=(n0 - n0 // 2, 1))
    outside = c + shell * np.linalg.norm(e)
    o0 = np.concatenate([inside, outside])
    d0 = unit_dirs(rng, n0)
    d0[len(inside):][::2] = (c + e * rng.uniform(-1, 1, size=(len(outside[::2]), 3))) - outside[::2]  # half of the outside rays aim into the scene
    first = oracle_rays(O, ps, o0, d0, O.MODE_FLAT, -1)
    hit = np.flatnonzero(first["id"] >= 0)
    assert len(hit) > n0 // 50, "the first batch must find surfaces to start from"
    pick = hit[rng.integers(0, len(hit), size=(n - n0) // 2)]
    p, nrm, din = first["point"][pick], first["normal"][pick], d0[pick] / np.linalg.norm(d0[pick], axis=1)[:, None]
    refl = din - 2.0 * np.sum(din * nrm, axis=1)[:, None] * nrm
    o = np.concatenate([o0, p, p])
    d = np.concatenate([d0, nrm, refl])
    with np.errstate(all="ignore"):
        unusable = ~(np.isfinite(d).all(axis=1) & (np.linalg.norm(d, axis=1) > 1e-12))  # (a degenerate normal of the first batch)
    d[unusable] = (0.0, 1.0, 0.0)
    d = d * (10.0 ** rng.uniform(-3, 3, size=(len(d), 1))) / np.linalg.norm(d, axis=1)[:, None]   # lengths over [1e-3, 1e3]
    m = len(d)
    ax = rng.choice(m, size=m // 16, replace=False)           # a share exactly axis-parallel: one component, the others +0 or -0
    length = np.linalg.norm(d[ax], axis=1)
    d[ax] = np.where(rng.random((len(ax), 3)) < 0.5, 0.0, -0.0)
    d[ax, rng.integers(0, 3, size=len(ax))] = length * rng.choice([-1.0, 1.0], size=len(ax))
    mz = rng.choice(m, size=m // 16, replace=False)           # a share with one -0 component
    d[mz, rng.integers(0, 3, size=len(mz))] = -0.0
    dead = ~np.any(d != 0.0, axis=1)
    d[dead] = (1.0, 0.0, -0.0)
    order = rng.permutation(m)                                # seeded random order: wavefronts mix everything
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    assert np.isfinite(o).all() and np.isfinite(d).all() and np.any(d != 0.0, axis=1).all()
    octs = (d[:, 0] < 0) * 1 + (d[:, 1] < 0) * 2 + (d[:, 2] < 0) * 4
    mixed = sum(len(np.unique(octs[k:k + 64])) > 1 for k in range(0, m - 63, 64))
    assert mixed > 0.99 * (m // 64), "nearly every wavefront must mix octants"
    return o, d


def load_scene(O, host, which):
    """(host scene, packed oracle scene, mesh triangle offsets, k-d depth) of "name" (an example scene) or "random:k" / "extreme:k"."""
    if ":" in which and which.split(":")[0] in ("random", "extreme"):
        from fuzz_gpu_parity import extreme_scene
        from test_gpu_render_parity import random_scene
        kind, k = which.split(":")
        scene, _ = (random_scene if kind == "random" else extreme_scene)(int(k))
        ps = O.pack(scene)
        return host_glue.host_scene(scene), ps, packed_tri_off(ps.arrays), 8
    sc = host.Scene.example(which, assets=ASSETS)
    a = sc.export()
    return sc, O.pack_arrays(a), packed_tri_off(a), 10


def flat_of(O, ps, tri_off):
    flat = O.flatten(ps)
    flat["_mesh_tri_off"] = tri_off
    flat["material_expected"] = first_use_order(flat["material"])
    return flat


def same(a, b, keys=ALL):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- 1. camera rays: Renderer.rays == Renderer.aov == the oracle
@pytest.mark.parametrize("name", ["primitives", "simple-cows", "robot-alarm-clock"])
def test_camera_rays_equal_the_primary_visibility_pass_and_the_oracle(oracle, host, H, name):
    sc, ps, tri_off, kd = load_scene(oracle, host, name)
    flat = flat_of(oracle, ps, tri_off)
    ys, xs = np.mgrid[0:HT, 0:W]
    o, d = oracle.camera_rays(sc.camera, W, HT, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(sc, tr, kd_depth=kd)
        aov = r.aov(sc.camera, W, HT)
        got = r.rays(o, d)
        r.close()
        for k, ka in (("t", "depth"), ("position", "position"), ("normal", "normal"), ("node", "node"), ("sub", "sub"), ("material", "material")):
            assert got[k].tobytes() == aov[ka].tobytes(), f"{name} {mname}: {k} != aov's {ka}"
        assert np.array_equal(got["occluded"], (got["node"] >= 0).astype(np.uint8))
        ref = {k: v.reshape(-1, *v.shape[2:]) for k, v in oracle_aov(oracle, ps, sc.camera, W, HT, om, kd).items()}
        compare(f"{name} {mname} camera rays", as_aov(got), ref, flat, hier=mname == "hier")


# ---- 2. incoherent rays, and 4. occlusion on the same batches
INCOHERENT = ["primitives", "hier", "instance", "simple-cows", "robot-alarm-clock", "big-scene", "soft-shadows", "random:2", "extreme:3"]


@pytest.mark.parametrize("which", INCOHERENT)
def test_incoherent_rays_match_the_oracle_in_every_traversal(oracle, host, H, which):
    sc, ps, tri_off, kd = load_scene(oracle, host, which)
    flat = flat_of(oracle, ps, tri_off)
    o, d = incoherent_batch(oracle, ps, flat, seed=sum(map(ord, which)))
    flat_node = None
    for mname, tr, om in modes(H, oracle):
        ref = oracle_rays(oracle, ps, o, d, om, kd)
        r = host.Renderer(sc, tr, kd_depth=kd)
        got = r.rays(o, d)
        again = r.rays(o, d, reorder=True)
        occ = [r.rays(o, d, any_hit=True, reorder=ro)["occluded"] for ro in (False, True)]
        r.close()
        hit = ref["id"] >= 0
        print(f"{which} {mname}: {len(o)} rays, {int(hit.sum())} hits")
        assert hit.sum() > len(o) // 50
        same_in_hier = which == "soft-shadows" and mname == "hier"  # no transformed groups: hierarchical and flat_scene agree
        compare(f"{which} {mname}", as_aov(got), ref, flat, hier=mname == "hier", flat_node=flat_node if same_in_hier else None)
        assert np.array_equal(got["occluded"], hit.astype(np.uint8))
        same(got, again)
        for ro, x in zip((0, 1), occ):
            assert np.array_equal(x, hit.astype(np.uint8)), f"{which} {mname}: any_hit (reorder={ro}) != (oracle id >= 0)"
        if mname == "flat":
            flat_node = got["node"]


@pytest.mark.parametrize("cache", [None, "0"])
def test_shadow_rays_of_a_render_are_occluded_where_the_oracle_hits(oracle, host, H, monkeypatch, cache):
    """Rays from big-scene's primary hit points toward each of its lights: the shadow rays of a render (material.rs:171-179)."""
    if cache is not None:
        monkeypatch.setenv("PORTRAYER_SHADOW_CACHE", cache)
    sc, ps, tri_off, kd = load_scene(oracle, host, "big-scene")
    lights = np.asarray(sc.export()["lights"]).reshape(-1, 15)[:, :3]
    assert len(lights) >= 2
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(sc, tr, kd_depth=kd)
        bg = default_background(W, HT)
        r.render(sc.camera, W, HT, bg, samples=1)  # (a render first: the occluder table of its shadow rays exists, or with the variable set does not)
        prim = r.aov(sc.camera, W, HT, want=("position", "node"))
        p = prim["position"][prim["node"] >= 0]
        assert len(p) > 5000
        o = np.ascontiguousarray(np.repeat(p, len(lights), axis=0))
        to = np.tile(lights, (len(p), 1)) - o
        d = np.ascontiguousarray(to / np.linalg.norm(to, axis=1)[:, None])
        got = [r.rays(o, d, any_hit=True, reorder=ro)["occluded"] for ro in (False, True)]
        r.close()
        ref = oracle_rays(oracle, ps, o, d, om, kd)["id"] >= 0
        print(f"big-scene {mname} shadow rays: {len(o)}, {int(ref.sum())} occluded")
        assert 0 < ref.sum() < len(o)
        for x in got:
            assert np.array_equal(x, ref.astype(np.uint8)), mname


# ---- 3. schedule independence
@pytest.mark.parametrize("which,mname", [("big-scene", "flat"), ("big-scene", "kd"), ("simple-cows", "hier"), ("robot-alarm-clock", "kd"), ("robot-alarm-clock", "flat"), ("instance", "hier")])
def test_no_result_depends_on_which_rays_share_a_wavefront(oracle, host, H, which, mname):
    sc, ps, tri_off, kd = load_scene(oracle, host, which)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=7, n=30_000)
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    r = host.Renderer(sc, tr, kd_depth=kd)
    base = r.rays(o, d)
    assert (base["node"] >= 0).sum() > 1000
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(o))
    for ro in (False, True):
        got = r.rays(np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), reorder=ro)
        same(got, {k: base[k][perm] for k in ALL})
    for n in (1, 63, 64, 65, 12_345):
        for ro in (False, True):
            got = r.rays(o[:n].copy(), d[:n].copy(), reorder=ro)
            same(got, {k: base[k][:n] for k in ALL})
    o2, d2 = o.copy(), d.copy()
    o2[::2], d2[::2] = o[0], d[0]  # every other ray a copy of ray 0
    for ro in (False, True):
        got = r.rays(o2, d2, reorder=ro)
        want = {k: base[k].copy() for k in ALL}
        for k in ALL:
            want[k][::2] = base[k][0]
        same(got, want)
    r.close()


# ---- 5. invalid rays
@pytest.mark.parametrize("which,mname", [("big-scene", "flat"), ("simple-cows", "kd"), ("robot-alarm-clock", "hier")])
def test_invalid_rays_miss_and_disturb_no_other_ray(oracle, host, H, which, mname):
    sc, ps, tri_off, kd = load_scene(oracle, host, which)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=19, n=30_000)
    rng = np.random.default_rng(23)
    n_bad = 997
    at = np.sort(rng.choice(len(o), size=n_bad, replace=False))  # np.insert: bad ray k goes in front of valid ray at[k]
    bo, bd = o[rng.integers(0, len(o), size=n_bad)].copy(), d[rng.integers(0, len(o), size=n_bad)].copy()
    kind = rng.integers(0, 6, size=n_bad)
    comp = rng.integers(0, 3, size=n_bad)
    for k in range(n_bad):
        if kind[k] == 0: bo[k, comp[k]] = np.nan
        elif kind[k] == 1: bd[k, comp[k]] = np.nan
        elif kind[k] == 2: bo[k, comp[k]] = np.inf if k % 2 else -np.inf
        elif kind[k] == 3: bd[k, comp[k]] = np.inf if k % 2 else -np.inf
        elif kind[k] == 4: bd[k] = (0.0, -0.0, 0.0)
        else: bd[k, comp[k]] = 3e18 if k % 2 else -1e300  # beyond the range the header states
    assert len(np.unique(kind)) == 6
    o2, d2 = np.insert(o, at, bo, axis=0), np.insert(d, at, bd, axis=0)
    bad = np.zeros(len(o2), dtype=bool)
    bad[at + np.arange(n_bad)] = True
    assert bad.sum() == n_bad and np.array_equal(o2[~bad], o) and np.array_equal(bits(d2[~bad]), bits(d))
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    r = host.Renderer(sc, tr, kd_depth=kd)
    base = r.rays(o, d)
    base_occ = r.rays(o, d, any_hit=True)["occluded"]
    assert (base["node"] >= 0).sum() > 1000
    for ro in (False, True):
        got = r.rays(o2, d2, reorder=ro)
        same({k: got[k][~bad] for k in ALL}, base)
        assert np.all(np.isposinf(got["t"][bad])) and np.all(got["node"][bad] == -1) and np.all(got["sub"][bad] == -1) and np.all(got["material"][bad] == -1)
        assert not got["occluded"][bad].any() and not bits(got["position"][bad]).any() and not bits(got["normal"][bad]).any()
        occ = r.rays(o2, d2, any_hit=True, reorder=ro)["occluded"]
        assert np.array_equal(occ[~bad], base_occ) and not occ[bad].any()
    only_bad = r.rays(np.ascontiguousarray(o2[bad][:200]), np.ascontiguousarray(d2[bad][:200]))  # wavefronts without a single ray
    assert np.all(only_bad["node"] == -1) and np.all(np.isposinf(only_bad["t"]))
    r.close()


# ---- 6. deep trees
def test_the_device_built_tree_of_a_million_triangles(oracle, host, H):
    """big-soup (1.25 M triangles, tree built on the device): its 40 x 24 camera rays and as many from the hit points back along the normals, shuffled."""
    w, h = 40, 24
    sc = host.Scene.example("synthetic:big-soup", n=6, assets=ASSETS)
    ps = oracle.pack_arrays(sc.export())
    ys, xs = np.mgrid[0:h, 0:w]
    o, d = oracle.camera_rays(sc.camera, w, h, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    first = oracle_rays(oracle, ps, o, d, oracle.MODE_FLAT, -1)
    hit = first["id"] >= 0
    assert hit.sum() > 100, "the camera must see the soup"
    o = np.concatenate([o, first["point"][hit]])
    d = np.concatenate([d, first["normal"][hit] * 0.037])
    order = np.random.default_rng(5).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    ref = oracle_rays(oracle, ps, o, d, oracle.MODE_FLAT, -1)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    for ro in (False, True):
        got = r.rays(o, d, reorder=ro, want=("t", "node", "position"))
        assert np.array_equal(bits(got["t"]), bits(ref["t"])) and np.array_equal(got["node"], ref["id"])
        assert np.array_equal(bits(got["position"])[ref["id"] >= 0], bits(ref["point"])[ref["id"] >= 0])
    r.close()


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
def test_a_stack_deeper_than_lds_is_walked_not_refused(oracle, host, H, monkeypatch, mode):
    """PORTRAYER_STACK_CAP=450 (the fixture of test_gpu_aov's test of this name): pt_test_cast_rays refuses the scene with PT_ERR_SCENE, the pass walks it."""
    from test_gpu_render_parity import random_scene
    scene, cam = random_scene(3)
    ps = oracle.pack(scene)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, packed_tri_off(ps.arrays)), seed=3, n=30_000)
    tr, om = {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]
    monkeypatch.setenv("PORTRAYER_STACK_CAP", "450")
    r = host.Renderer(host_glue.host_scene(scene), tr, kd_depth=8)
    rc = cast_one_ray(H, oracle, r.context, host_glue.cam10(cam), W, HT)
    assert rc == H.ERR_SCENE and b"too deep" in H.lib().pt_last_error(r.context), (rc, H.lib().pt_last_error(r.context))
    got = [r.rays(o, d, reorder=ro) for ro in (False, True)]
    occ = r.rays(o, d, any_hit=True)["occluded"]
    r.close()
    ref = oracle_rays(oracle, ps, o, d, om, 8)
    hit = ref["id"] >= 0
    assert hit.sum() > 1000
    same(got[0], got[1])
    assert np.array_equal(bits(got[0]["t"]), bits(ref["t"])) and np.array_equal(got[0]["node"] >= 0, hit) and np.array_equal(occ, hit.astype(np.uint8))
    assert np.array_equal(bits(got[0]["position"])[hit], bits(ref["point"])[hit]) and np.array_equal(bits(got[0]["normal"])[hit], bits(ref["normal"])[hit])
    if mode != "hier":
        assert np.array_equal(got[0]["node"], ref["id"])


# ---- 7. device path
def test_device_buffers_on_a_stream_equal_the_host_path(H):
    """pt_rays_device with rays and results in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first."""
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
sc = host.Scene.example("simple-cows", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
rng = np.random.default_rng(1)
n = 50_001
o = rng.uniform(-6, 6, size=(n, 3)); d = rng.normal(size=(n, 3))
pos = r.aov(sc.camera, 203, 117, want=("position", "node"))
p = pos["position"][pos["node"] >= 0]
o[:len(p)] = p
TORCH = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8}
PTR = {np.float64: H._dp, np.int32: H._ip, np.uint8: H._u8p}
for any_hit, reorder in ((0, 0), (0, 1), (1, 0), (1, 1)):
    names = ("occluded",) if any_hit else tuple(H.RAYS_BUFFERS)
    ref = r.rays(o, d, any_hit=bool(any_hit), reorder=bool(reorder))
    assert ref["occluded"].sum() > 1000
    t = {k: torch.full((n,) + ((3,) if H.RAYS_BUFFERS[k][1] == 3 else ()), 5, dtype=TORCH[H.RAYS_BUFFERS[k][0]], device=dev) for k in names}
    d_o, d_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    b = H.PtRaysBuffers()
    for k in names:
        setattr(b, k, C.cast(C.c_void_p(t[k].data_ptr()), PTR[H.RAYS_BUFFERS[k][0]]))
    p = H.PtRaysParams(n, any_hit, reorder)
    args = (r.context, C.byref(p), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_d.data_ptr()), C.byref(b), C.c_void_p(stream.cuda_stream))
    assert lib.pt_rays_device(*args) == H.OK, lib.pt_last_error(r.context)
    assert lib.pt_rays_device(*args) == H.ERR_ARGUMENT  # one pass in flight per context
    tt = np.zeros(n)
    hb = H.PtRaysBuffers(occluded=np.zeros(n, dtype=np.uint8).ctypes.data_as(H._u8p))
    assert lib.pt_rays(r.context, C.byref(p), o.ctypes.data_as(H._dp), d.ctypes.data_as(H._dp), C.byref(hb), None) == H.ERR_ARGUMENT  # ... the host path included
    ms = C.c_double(-1.0)
    assert lib.pt_rays_finish(r.context, C.byref(ms)) == H.OK and ms.value > 0.0
    assert lib.pt_rays_finish(r.context, None) == H.ERR_ARGUMENT  # nothing in flight any more
    stream.synchronize()
    for k in names:
        assert t[k].cpu().numpy().tobytes() == ref[k].tobytes(), (k, any_hit, reorder)
r.close()
assert (x * 2).sum().item() == 2048.0
print("rays into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rays into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_renders_and_an_aov_pass_queued_around_a_ray_pass_are_unchanged(oracle, host, H):
    """pt_render_device on both slots and a pt_aov_device pass in flight, then a ray pass on a stream of its own and a synchronous one, then everything is
    closed: every result equals what the same calls give one after the other on a second context."""
    import device_glue
    from example_scenes import EXAMPLES
    w, h, samples = 160, 96, 4
    bg = default_background(w, h)
    scene, cam0, _ = EXAMPLES["macho-cows"]()
    lib = H.lib()
    ys, xs = np.mgrid[0:h, 0:w]
    o, d = oracle.camera_rays(cam0, w, h, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))
    order = np.random.default_rng(2).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    n = len(o)
    camera = device_glue.camera_struct(cam0, w, h)
    results = []
    for overlapped in (False, True):
        ds = device_glue.DeviceScene(scene, H.TRAVERSE_FLAT)
        ctx = H.Context()
        ds.upload(ctx)
        c = ctx.handle

        def dev(nbytes):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0
            return p
        d_bg = dev(bg.nbytes)
        assert lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        d_img, d_depth, d_node, d_o, d_d, d_t, d_id = dev(w * h * 3), dev(w * h * 8), dev(w * h * 4), dev(n * 24), dev(n * 24), dev(n * 8), dev(n * 4)
        d_img2 = dev(w * h * 3)
        assert lib.pt_copy_to_device(c, d_o, o.ctypes.data_as(C.c_void_p), n * 24) == 0 and lib.pt_copy_to_device(c, d_d, d.ctypes.data_as(C.c_void_p), n * 24) == 0
        st = H.PtStats()
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp), node=C.cast(d_node, H._ip))
        rp = H.PtRaysParams(n, 0, 1)
        rb = H.PtRaysBuffers(t=C.cast(d_t, H._dp), node=C.cast(d_id, H._ip))
        host_occ = np.zeros(n, dtype=np.uint8)
        hp, hb = H.PtRaysParams(n, 1, 0), H.PtRaysBuffers(occluded=host_occ.ctypes.data_as(H._u8p))

        def render(k, img):
            p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, img, C.c_void_p(lib.pt_context_stream(c, k))) == 0, lib.pt_last_error(c)
        steps = [lambda: render(0, d_img), lambda: lib.pt_render_finish(c, C.byref(st)),
                 lambda: render(1, d_img2), lambda: lib.pt_render_finish(c, C.byref(st)),
                 lambda: lib.pt_aov_device(c, C.byref(camera), C.byref(ap), C.byref(ab), None), lambda: lib.pt_aov_finish(c, None),
                 lambda: lib.pt_rays_device(c, C.byref(rp), d_o, d_d, C.byref(rb), C.c_void_p(lib.pt_context_stream(c, 0))), lambda: lib.pt_rays_finish(c, None)]
        if overlapped:  # everything queued first, the synchronous ray pass in the middle of it, then closed oldest first
            for k in (0, 2, 4, 6):
                assert steps[k]() in (None, 0), lib.pt_last_error(c)
            assert lib.pt_rays(c, C.byref(hp), o.ctypes.data_as(H._dp), d.ctypes.data_as(H._dp), C.byref(hb), None) == H.ERR_ARGUMENT  # a device pass is in flight
            assert lib.pt_rays_finish(c, None) == 0, lib.pt_last_error(c)
            assert lib.pt_rays(c, C.byref(hp), o.ctypes.data_as(H._dp), d.ctypes.data_as(H._dp), C.byref(hb), None) == 0, lib.pt_last_error(c)
            for k in (1, 3, 5):
                assert steps[k]() == 0, lib.pt_last_error(c)
        else:
            for s in steps:
                assert s() in (None, 0), lib.pt_last_error(c)
            assert lib.pt_rays(c, C.byref(hp), o.ctypes.data_as(H._dp), d.ctypes.data_as(H._dp), C.byref(hb), None) == 0, lib.pt_last_error(c)
        out = {}
        for name, ptr, arr in (("img", d_img, np.zeros((h, w, 3), dtype=np.uint8)), ("img2", d_img2, np.zeros((h, w, 3), dtype=np.uint8)), ("depth", d_depth, np.zeros((h, w))),
                               ("node", d_node, np.zeros((h, w), dtype=np.int32)), ("t", d_t, np.zeros(n)), ("id", d_id, np.zeros(n, dtype=np.int32))):
            assert lib.pt_copy_from_device(c, arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
            out[name] = arr
        out["occ"] = host_occ
        for p in (d_bg, d_img, d_img2, d_depth, d_node, d_o, d_d, d_t, d_id):
            lib.pt_device_free(c, p)
        ctx.close()
        results.append(out)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), k
    assert (results[1]["id"] >= 0).sum() > 1000 and results[1]["img"].any()
    # and the ray pass is the aov pass on the same (shuffled) rays
    assert np.array_equal(bits(results[1]["t"]), bits(results[1]["depth"].ravel()[order])) and np.array_equal(results[1]["id"], results[1]["node"].ravel()[order])
    assert np.array_equal(results[1]["occ"], (results[1]["id"] >= 0).astype(np.uint8))


# ---- 8. single buffers
@pytest.mark.parametrize("name,traverse", [("primitives", "hier"), ("simple-cows", "flat"), ("robot-alarm-clock", "kd")])
def test_every_single_buffer_request_equals_the_all_buffers_request(oracle, host, H, name, traverse):
    sc, ps, tri_off, kd = load_scene(oracle, host, name)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=31, n=20_000)
    r = host.Renderer(sc, {"flat": H.TRAVERSE_FLAT, "kd": H.TRAVERSE_KD, "hier": H.TRAVERSE_HIER}[traverse], kd_depth=kd)
    full = r.rays(o, d)
    assert set(full) == set(ALL) | {"kernel_ms"} and (full["node"] >= 0).sum() > 500
    for ro in (False, True):
        for k in ALL:
            one = r.rays(o, d, want=(k,), reorder=ro)
            assert set(one) == {k, "kernel_ms"}
            assert one[k].tobytes() == full[k].tobytes(), k
        two = r.rays(o, d, want=("t", "node"), reorder=ro)
        assert two["t"].tobytes() == full["t"].tobytes() and two["node"].tobytes() == full["node"].tobytes()
    into = {"t": np.full(len(o), -7.25), "node": np.full(len(o), -7, dtype=np.int32)}
    back = r.rays(o, d, want=("t", "node"), into=into)
    assert back["t"] is into["t"] and into["t"].tobytes() == full["t"].tobytes() and into["node"].tobytes() == full["node"].tobytes()
    r.close()


def test_argument_errors(host, H):
    lib = H.lib()
    sc = host.Scene.example("primitives", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ctx = r.context
    n = 100
    o, d = np.zeros((n, 3)), np.ones((n, 3))
    t, occ = np.full(n, 3.0), np.full(n, 3, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    tb, ob = H.PtRaysBuffers(t=dp(t)), H.PtRaysBuffers(occluded=occ.ctypes.data_as(H._u8p))
    good = H.PtRaysParams(n, 0, 0)
    for fn, tail in ((lib.pt_rays, None), (lib.pt_rays_device, None)):
        assert fn(ctx, None, dp(o), dp(d), C.byref(tb), tail) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(d), C.byref(tb), tail) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), None, C.byref(tb), tail) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), dp(d), C.byref(H.PtRaysBuffers()), tail) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), dp(d), None, tail) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(H.PtRaysParams(H.RAYS_MAX + 1, 0, 0)), dp(o), dp(d), C.byref(tb), tail) == H.ERR_ARGUMENT
        for a, ro in ((2, 0), (-1, 0), (0, 2), (0, -1)):
            assert fn(ctx, C.byref(H.PtRaysParams(n, a, ro)), dp(o), dp(d), C.byref(ob), tail) == H.ERR_ARGUMENT, (a, ro)
        assert fn(ctx, C.byref(H.PtRaysParams(n, 1, 0)), dp(o), dp(d), C.byref(tb), tail) == H.ERR_ARGUMENT  # any_hit with more than `occluded`
        assert fn(ctx, C.byref(H.PtRaysParams(0, 0, 0)), dp(o), dp(d), C.byref(tb), tail) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(t == 3.0) and np.all(occ == 3)
    assert lib.pt_rays_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    assert lib.pt_rays(ctx, C.byref(good), dp(o), dp(d), C.byref(tb), None) == H.OK
    bare = H.Context()
    assert lib.pt_rays(bare.handle, C.byref(good), dp(o), dp(d), C.byref(tb), None) == H.ERR_NO_SCENE
    assert lib.pt_rays_device(bare.handle, C.byref(good), dp(o), dp(d), C.byref(tb), None) == H.ERR_NO_SCENE
    assert lib.pt_rays(bare.handle, C.byref(H.PtRaysParams(n, 3, 0)), dp(o), dp(d), C.byref(tb), None) == H.ERR_ARGUMENT  # the argument comes first
    bare.close()
    empty = r.rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty["t"].shape == (0,) and empty["position"].shape == (0, 3)
    r.close()


_OVERFLOW = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
from portrayer_amd import _hip as H
from portrayer_amd import host
sc = host.Scene.example("big-scene")
r = host.Renderer(sc, H.TRAVERSE_FLAT)
rng = np.random.default_rng(0)
try:
    r.rays(rng.uniform(-400, 400, size=(20000, 3)), rng.normal(size=(20000, 3)))
    print("NO ERROR")
except host.PortrayerHostError as e:
    print("ERR", e)
"""


def test_stack_overflow_is_an_error_not_a_wrong_answer():
    """PORTRAYER_STACK_CAP=2 makes the walk of a 1000-node scene run out of stack: PT_ERR_TRAVERSAL, as for a render and for pt_aov."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _OVERFLOW % root], env=dict(os.environ, PORTRAYER_STACK_CAP="2"), capture_output=True, text=True, timeout=300)
    assert "ERR" in out.stdout and "overflow" in out.stdout and "NO ERROR" not in out.stdout, out.stdout + out.stderr
