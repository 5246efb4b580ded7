"""The radiance pass (pt_radiance / pt_radiance_device / Renderer.radiance) against the oracle's po_color_rays and po_render and against pt_render, bit for bit.

Every comparison in this file is exact: bits() equality of f64. No ray is left out of a comparison except the invalid rays a test injects itself, whose number it
knows and asserts, and - for the ORACLE comparison of scenes that texture or normal-map a sphere only - renders in which the oracle counts a sphere texture
coordinate near a texel edge (tests/test_gpu_textures.py: texel_edge_proof); the comparison with pt_render is unconditional."""
import ctypes as C
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import host_glue  # noqa: E402
from scene_dsl import ASSETS, default_background  # noqa: E402
from test_gpu_aov import bits, modes, packed_tri_off  # noqa: E402
from test_gpu_rays import flat_of, incoherent_batch, load_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W, HT = 67, 37  # a multiple of 8 (and of 64) in neither direction
BG = (0.25, 0.5, 0.75)
SPHERE = 0  # PT_PRIM_SPHERE


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def oracle_color(O, ps, o, d, mode, kd_depth, background=BG, workers=16):
    """po_color_rays over the batch (seed 0, sample 0, one background colour), split over `workers` host threads. po_color_rays draws for the ray at index i of
    ITS call from stream (0, i, 0), so a part [k, k + m) is handed over behind k placeholder rays that start far outside every scene and point away from it
    (they cost a miss each, their colours are dropped): every ray keeps the index, and so the stream, it has in the whole batch."""
    parts = [p for p in np.array_split(np.arange(len(o)), workers) if len(p)]
    far_o, far_d = np.array([3e7, 5e7, 7e7]), np.array([0.267, 0.535, 0.802])

    def one(p):
        k = int(p[0])
        oo = np.concatenate([np.tile(far_o, (k, 1)), o[p]])
        dd = np.concatenate([np.tile(far_d, (k, 1)), d[p]])
        return O.color_rays(ps, oo, dd, background=background, mode=mode, kd_depth=kd_depth)[k:]
    with ThreadPoolExecutor(max_workers=workers) as ex:
        res = list(ex.map(one, parts))
    return np.concatenate(res)


def pixel_centre_rays(O, cam, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return O.camera_rays(cam, w, h, np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1).astype(np.float64))


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, what
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def all_examples():
    from example_scenes import EXAMPLES, MORE_EXAMPLES, TEXTURED_EXAMPLES
    return {**EXAMPLES, **MORE_EXAMPLES, **TEXTURED_EXAMPLES}


def example_names():
    from example_scenes import EXAMPLES, MORE_EXAMPLES, TEXTURED_EXAMPLES
    return list(EXAMPLES) + list(MORE_EXAMPLES) + list(TEXTURED_EXAMPLES)


# ---- 1. camera rays: radiance == po_color_rays == po_render == pt_render
@pytest.mark.parametrize("name", example_names())
def test_pixel_centre_rays_equal_the_oracle_and_the_render(oracle, host, H, name):
    scene, cam, _ = all_examples()[name]()
    ps = oracle.pack(scene)
    hs, c10 = host_glue.host_scene(scene), host_glue.cam10(cam)
    o, d = pixel_centre_rays(oracle, cam, W, HT)
    bg_px = np.random.default_rng(sum(map(ord, name))).uniform(0.0, 1.0, size=(HT, W, 3))
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        for seed in (0, 7):
            ref = oracle.render(ps, cam, W, HT, background=bg_px, samples=1, seed=seed, jitter=oracle.JITTER_CENTRE, mode=om, kd_depth=8)
            sphere_maps_exact = ref.stats["tex_sphere_near_edge"] == 0  # (0 lookups in scenes without a mapped sphere)
            got = r.radiance(o, d, background=bg_px.reshape(-1, 3), seed=seed)["rgb"]
            _, linear, _ = r.render(c10, W, HT, bg_px, samples=1, seed=seed, sample_mode=H.SAMPLE_CENTRE)
            same_bits(got, linear.reshape(-1, 3), f"{name} {mname} seed {seed}: radiance vs pt_render linear")
            if sphere_maps_exact:
                same_bits(got, ref.linear.reshape(-1, 3), f"{name} {mname} seed {seed}: radiance vs po_render linear")
            if seed == 0:
                const = r.radiance(o, d, background=BG)["rgb"]
                if sphere_maps_exact:
                    same_bits(const, oracle_color(oracle, ps, o, d, om, 8), f"{name} {mname}: radiance vs po_color_rays")
                hit_something = ~np.all(const == np.array(BG), axis=1)
                assert hit_something.sum() > 50, "the camera must see the scene"
        r.close()


# ---- 2. the sample index
@pytest.mark.parametrize("name", ["glossy-reflection", "soft-shadows", "entering-the-mirror-dimension"])
def test_four_samples_added_in_order_equal_a_four_sample_render(oracle, host, H, name):
    """The chunk contract sums fewer than 8 samples in ascending order and the division by 4 is exact: numpy's ((s0 + s1) + s2) + s3) / 4 is the render's mean."""
    scene, cam, _ = all_examples()[name]()
    ps = oracle.pack(scene)
    hs = host_glue.host_scene(scene)
    o, d = pixel_centre_rays(oracle, cam, W, HT)
    bg = default_background(W, HT)
    bg_rays = np.ascontiguousarray(np.repeat(bg, W, axis=0))
    differs = False
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        s = [r.radiance(o, d, background=bg_rays, seed=5, sample=k)["rgb"] for k in range(4)]
        r.close()
        mean = (((s[0] + s[1]) + s[2]) + s[3]) / 4.0
        ref = oracle.render(ps, cam, W, HT, background=bg, samples=4, seed=5, jitter=oracle.JITTER_CENTRE, mode=om, kd_depth=8)
        same_bits(mean, ref.linear.reshape(-1, 3), f"{name} {mname}: mean of samples 0..3")
        differs = differs or not np.array_equal(bits(s[0]), bits(s[1]))
    assert differs == (name != "entering-the-mirror-dimension"), "the sample index matters exactly where the scene draws (glossy material, area light)"


# ---- 3. incoherent batches
INCOHERENT = ["primitives-simple", "big-scene", "entering-the-mirror-dimension", "glossy-reflection", "soft-shadows", "macho-cows", "hier", "fish"]


def test_the_textured_scene_of_the_incoherent_batches_maps_no_sphere(host):
    """fish: a textured mesh. No node that carries a textured or normal-mapped material is a sphere, so no texture coordinate goes through atan2 / acos."""
    a = host.Scene.example("fish", assets=ASSETS).export()
    mapped = [m for m in range(len(a["material_texture"])) if a["material_texture"][m] >= 0 or a["material_normal_map"][m] >= 0]
    assert mapped, "fish has a textured material"
    prim, mat = np.asarray(a["prim_type"]), np.asarray(a["material"])
    assert np.isin(mat, mapped).any() and not (np.isin(mat, mapped) & (prim == SPHERE)).any()


@pytest.mark.parametrize("which", INCOHERENT)
def test_incoherent_rays_match_the_oracle_in_every_traversal(oracle, host, H, which):
    sc, ps, tri_off, kd = load_scene(oracle, host, which)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=sum(map(ord, which)))
    assert len(o) >= 99_000
    for mname, tr, om in modes(H, oracle):
        ref = oracle_color(oracle, ps, o, d, om, kd)
        r = host.Renderer(sc, tr, kd_depth=kd)
        got = r.radiance(o, d, background=BG)["rgb"]
        again = r.radiance(o, d, background=BG, reorder=True)["rgb"]
        r.close()
        shaded = ~np.all(ref == np.array(BG), axis=1)
        print(f"{which} {mname}: {len(o)} rays, {int(shaded.sum())} not the background")
        assert shaded.sum() > len(o) // 50
        same_bits(got, ref, f"{which} {mname}")
        same_bits(again, got, f"{which} {mname}: reorder = 1 vs 0")


# ---- 4. streams
@pytest.mark.parametrize("which,mname", [("soft-shadows", "flat"), ("glossy-reflection", "kd"), ("glossy-reflection", "hier"), ("big-scene", "flat")])
def test_a_cut_batch_with_its_stream_base_equals_the_slice_of_the_whole(oracle, host, H, which, mname):
    sc, ps, tri_off, kd = load_scene(oracle, host, which)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=7, n=30_000)
    bg = np.random.default_rng(3).uniform(size=(len(o), 3))
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    r = host.Renderer(sc, tr, kd_depth=kd)
    whole = r.radiance(o, d, background=bg, seed=9, sample=2, stream_base=1000)["rgb"]
    for k, m in ((0, 1), (0, 63), (63, 65), (64, 64), (12_345, len(o) - 12_345), (len(o) - 1, 1)):
        for ro in (False, True):
            part = r.radiance(o[k:k + m].copy(), d[k:k + m].copy(), background=bg[k:k + m].copy(), seed=9, sample=2, stream_base=1000 + k, reorder=ro)["rgb"]
            same_bits(part, whole[k:k + m], f"{which} {mname}: [{k}, {k + m}) reorder={ro}")
    r.close()


@pytest.mark.parametrize("mname", ["flat", "kd", "hier"])
def test_a_permuted_batch_equals_the_permuted_result_only_where_nothing_is_drawn(oracle, host, H, mname):
    """soft-shadows draws (an area light): ray i's draws come from stream stream_base + i, so moving a ray to another index changes its colour where the draws
    matter. primitives-simple draws nothing: only the grouping changes, and no result depends on it."""
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    perm = None
    for which, draws in (("soft-shadows", True), ("primitives-simple", False)):
        sc, ps, tri_off, kd = load_scene(oracle, host, which)
        o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, tri_off), seed=13, n=30_000)
        perm = np.random.default_rng(11).permutation(len(o))
        r = host.Renderer(sc, tr, kd_depth=kd)
        base = r.radiance(o, d, background=BG, seed=3)["rgb"]
        for ro in (False, True):
            got = r.radiance(np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]), background=BG, seed=3, reorder=ro)["rgb"]
            equal = np.array_equal(bits(got), bits(base[perm]))
            assert equal == (not draws), f"{which} {mname} reorder={ro}: permuted batch {'equals' if equal else 'differs from'} the permuted result"
            if draws:  # ... and the rays whose shading drew nothing (misses, unlit or fully shadowed hits) are unchanged all the same
                assert np.all(got[np.all(base[perm] == np.array(BG), axis=1)] == np.array(BG))
        r.close()


# ---- 5. invalid rays
@pytest.mark.parametrize("which,mname", [("big-scene", "flat"), ("macho-cows", "kd"), ("entering-the-mirror-dimension", "hier"), ("soft-shadows", "flat")])
def test_invalid_rays_report_their_background_and_disturb_no_other_ray(oracle, host, H, which, mname):
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
        else: bd[k, comp[k]] = 1e19 if k % 2 else -1e300  # beyond the range the header states
    assert len(np.unique(kind)) == 6
    o2, d2 = np.insert(o, at, bo, axis=0), np.insert(d, at, bd, axis=0)
    bad = np.zeros(len(o2), dtype=bool)
    bad[at + np.arange(n_bad)] = True
    assert bad.sum() == n_bad and np.array_equal(o2[~bad], o) and np.array_equal(bits(d2[~bad]), bits(d))
    bg2 = rng.uniform(size=(len(o2), 3))
    bg2[np.flatnonzero(bad)[::5]] = -0.0  # (a background of -0 bits comes back as -0)
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    r = host.Renderer(sc, tr, kd_depth=kd)
    # the valid rays alone, each on the stream it has in the batch with the invalid ones: stream_base + its index THERE. One pass per run of consecutive indices
    # would be 998 passes; instead the base is computed with the invalid rays replaced by valid ones (copies of ray 0), which by the contract disturbs nothing either.
    o3, d3 = o2.copy(), d2.copy()
    o3[bad], d3[bad] = o[0], d[0]
    base = r.radiance(o3, d3, background=bg2, seed=4)["rgb"]
    assert (~np.all(base[~bad] == bg2[~bad], axis=1)).sum() > 1000
    for ro in (False, True):
        got = r.radiance(o2, d2, background=bg2, seed=4, reorder=ro)["rgb"]
        same_bits(got[~bad], base[~bad], f"{which} {mname} reorder={ro}: valid rays")
        same_bits(got[bad], bg2[bad], f"{which} {mname} reorder={ro}: invalid rays report their background")
    only_bad = r.radiance(np.ascontiguousarray(o2[bad][:200]), np.ascontiguousarray(d2[bad][:200]), background=np.ascontiguousarray(bg2[bad][:200]))["rgb"]  # wavefronts without a single ray
    same_bits(only_bad, bg2[bad][:200], "only invalid rays")
    const = r.radiance(np.ascontiguousarray(o2[bad][:70]), np.ascontiguousarray(d2[bad][:70]), background=BG)["rgb"]
    same_bits(const, np.tile(np.array(BG), (70, 1)), "only invalid rays, one background colour")
    r.close()


# ---- 7. large scene, deep trees
def test_the_device_built_tree_of_a_million_triangles(oracle, host, H):
    """big-soup (1.25 M triangles, tree built on the device): its 40 x 24 camera rays and as many from the hit points back along the normals, shuffled."""
    from test_gpu_rays import oracle_rays
    w, h = 40, 24
    sc = host.Scene.example("synthetic:big-soup", n=6, assets=ASSETS)
    ps = oracle.pack_arrays(sc.export())
    o, d = pixel_centre_rays(oracle, sc.camera, w, h)
    first = oracle_rays(oracle, ps, o, d, oracle.MODE_FLAT, -1)
    hit = first["id"] >= 0
    assert hit.sum() > 100, "the camera must see the soup"
    o = np.concatenate([o, first["point"][hit]])
    d = np.concatenate([d, first["normal"][hit] * 0.037])
    order = np.random.default_rng(5).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    ref = oracle_color(oracle, ps, o, d, oracle.MODE_FLAT, -1)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    for ro in (False, True):
        same_bits(r.radiance(o, d, background=BG, reorder=ro)["rgb"], ref, f"big-soup reorder={ro}")
    r.close()


@pytest.mark.parametrize("mode", ["flat", "kd", "hier"])
def test_a_stack_deeper_than_lds_is_walked_not_refused(oracle, host, H, monkeypatch, mode):
    """PORTRAYER_STACK_CAP=450 (the fixture of test_gpu_rays' test of this name): pt_test_cast_rays refuses the scene with PT_ERR_SCENE, the pass walks it."""
    from test_gpu_aov import cast_one_ray
    from test_gpu_render_parity import random_scene
    scene, cam = random_scene(3)
    ps = oracle.pack(scene)
    o, d = incoherent_batch(oracle, ps, flat_of(oracle, ps, packed_tri_off(ps.arrays)), seed=3, n=30_000)
    tr, om = {"flat": (H.TRAVERSE_FLAT, oracle.MODE_FLAT), "kd": (H.TRAVERSE_KD, oracle.MODE_KD), "hier": (H.TRAVERSE_HIER, oracle.MODE_HIER)}[mode]
    monkeypatch.setenv("PORTRAYER_STACK_CAP", "450")
    r = host.Renderer(host_glue.host_scene(scene), tr, kd_depth=8)
    rc = cast_one_ray(H, oracle, r.context, host_glue.cam10(cam), 203, 117)
    assert rc == H.ERR_SCENE and b"too deep" in H.lib().pt_last_error(r.context), (rc, H.lib().pt_last_error(r.context))
    got = [r.radiance(o, d, background=BG, reorder=ro)["rgb"] for ro in (False, True)]
    r.close()
    ref = oracle_color(oracle, ps, o, d, om, 8)
    assert (~np.all(ref == np.array(BG), axis=1)).sum() > 1000
    same_bits(got[0], ref, f"deep stack {mode}")
    same_bits(got[1], got[0], f"deep stack {mode}: reorder")


# ---- 6. device path
def test_device_buffers_on_a_stream_equal_the_host_path(H):
    """pt_radiance_device with every array in torch tensors on a stream of torch's, in a process of its own in which torch initialises its GPU side first."""
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
sc = host.Scene.example("entering-the-mirror-dimension", assets=ASSETS)
r = host.Renderer(sc, H.TRAVERSE_FLAT)
rng = np.random.default_rng(1)
n = 50_001
o = rng.uniform(-6, 6, size=(n, 3)); d = rng.normal(size=(n, 3))
pos = r.aov(sc.camera, 203, 117, want=("position", "node"))
p = pos["position"][pos["node"] >= 0]
o[:len(p)] = p
bg = rng.uniform(size=(n, 3))
for per_ray, reorder in ((0, 0), (0, 1), (1, 0), (1, 1)):
    b = bg if per_ray else bg[0].copy()
    ref = r.radiance(o, d, background=b, seed=2, sample=1, stream_base=77, reorder=bool(reorder))["rgb"]
    assert (~np.all(ref == (bg if per_ray else bg[0]), axis=1)).sum() > 1000
    t = torch.full((n, 3), 5, dtype=torch.float64, device=dev)
    d_o, d_d, d_b = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    p = H.PtRadianceParams(n, reorder, per_ray, 2, 77, 1)
    args = (r.context, C.byref(p), C.c_void_p(d_o.data_ptr()), C.c_void_p(d_d.data_ptr()), C.c_void_p(d_b.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(stream.cuda_stream))
    assert lib.pt_radiance_device(*args) == H.OK, lib.pt_last_error(r.context)
    assert lib.pt_radiance_device(*args) == H.ERR_ARGUMENT  # one pass in flight per context
    hr = np.zeros((n, 3))
    dp = lambda a: a.ctypes.data_as(H._dp)
    assert lib.pt_radiance(r.context, C.byref(p), dp(o), dp(d), dp(np.ascontiguousarray(b)), dp(hr), None) == H.ERR_ARGUMENT  # ... the host path included
    ms = C.c_double(-1.0)
    assert lib.pt_radiance_finish(r.context, C.byref(ms)) == H.OK and ms.value > 0.0
    assert lib.pt_radiance_finish(r.context, None) == H.ERR_ARGUMENT  # nothing in flight any more
    stream.synchronize()
    assert t.cpu().numpy().tobytes() == ref.tobytes(), (per_ray, reorder)
    assert not hr.any()
r.close()
assert (x * 2).sum().item() == 2048.0
print("radiance into torch tensors ok")
""" % (root, root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "radiance into torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_renders_an_aov_pass_and_a_rays_pass_in_flight_around_a_radiance_pass_are_unchanged(oracle, host, H, monkeypatch):
    """Three queues at work at once: a render on the context's stream 0; the rays pass and then the second render on its stream 1; the aov pass and then the radiance
    pass on the NULL stream (the context's streams are non-blocking: nothing orders them against it). The mirror scene parks recursion frames, so the context would
    hand out ONE stream for both slots: PORTRAYER_TWO_STREAMS=1 makes them two. The frames are large enough (640 x 360 x 16 samples) for the renders to be
    running while the radiance pass runs, is closed, and a synchronous host-buffer pass follows it. Every result equals what the same calls give one after the
    other on a second context - which they would not if the pass shared a stack column, a frame line or a queue with a slot or another pass."""
    import device_glue
    from example_scenes import EXAMPLES
    monkeypatch.setenv("PORTRAYER_TWO_STREAMS", "1")
    w, h, samples = 640, 360, 16
    bg = default_background(w, h)
    scene, cam0, _ = EXAMPLES["entering-the-mirror-dimension"]()
    lib = H.lib()
    o, d = pixel_centre_rays(oracle, cam0, w, h)
    order = np.random.default_rng(2).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    n = len(o)
    bg_rays = np.ascontiguousarray(np.repeat(bg, w, axis=0)[order])
    camera = device_glue.camera_struct(cam0, w, h)
    results = []
    for overlapped in (False, True):
        ds = device_glue.DeviceScene(scene, H.TRAVERSE_FLAT)
        ctx = H.Context()
        ds.upload(ctx)
        c = ctx.handle

        def dev(nbytes, src=None):
            p = C.c_void_p()
            assert lib.pt_device_alloc(c, nbytes, C.byref(p)) == 0
            if src is not None:
                assert lib.pt_copy_to_device(c, p, src.ctypes.data_as(C.c_void_p), src.nbytes) == 0
            return p
        d_bg, d_o, d_d, d_bgr = dev(bg.nbytes, bg), dev(n * 24, o), dev(n * 24, d), dev(n * 24, bg_rays)
        d_img, d_img2, d_depth, d_node, d_t, d_id, d_rad = dev(w * h * 3), dev(w * h * 3), dev(w * h * 8), dev(w * h * 4), dev(n * 8), dev(n * 4), dev(n * 24)
        st = H.PtStats()
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp), node=C.cast(d_node, H._ip))
        rp = H.PtRaysParams(n, 0, 1)
        rb = H.PtRaysBuffers(t=C.cast(d_t, H._dp), node=C.cast(d_id, H._ip))
        qp = H.PtRadianceParams(n, 1, 1, 6, 0, 0)
        host_rad = np.zeros((n, 3))
        hp = H.PtRadianceParams(n, 0, 0, 6, 0, 1)
        hbg = np.array(BG)
        dp = lambda a: a.ctypes.data_as(H._dp)

        def render(k, img):
            p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, img, C.c_void_p(lib.pt_context_stream(c, k))) == 0, lib.pt_last_error(c)
        assert lib.pt_context_stream(c, 0) != lib.pt_context_stream(c, 1) and lib.pt_context_stream(c, 0) and lib.pt_context_stream(c, 1)
        steps = [lambda: render(0, d_img), lambda: lib.pt_render_finish(c, C.byref(st)),
                 lambda: lib.pt_rays_device(c, C.byref(rp), d_o, d_d, C.byref(rb), C.c_void_p(lib.pt_context_stream(c, 1))), lambda: lib.pt_rays_finish(c, None),
                 lambda: render(1, d_img2), lambda: lib.pt_render_finish(c, C.byref(st)),
                 lambda: lib.pt_aov_device(c, C.byref(camera), C.byref(ap), C.byref(ab), None), lambda: lib.pt_aov_finish(c, None),
                 lambda: lib.pt_radiance_device(c, C.byref(qp), d_o, d_d, d_bgr, d_rad, None), lambda: lib.pt_radiance_finish(c, None)]
        host_pass = lambda: lib.pt_radiance(c, C.byref(hp), dp(o), dp(d), dp(hbg), dp(host_rad), None)
        if overlapped:  # everything queued first on its three queues; the radiance pass closed and a synchronous one run while the renders and the rays pass are open
            for k in (0, 2, 4, 6, 8):
                assert steps[k]() in (None, 0), lib.pt_last_error(c)
            assert host_pass() == H.ERR_ARGUMENT  # a device pass is in flight
            assert lib.pt_radiance_finish(c, None) == 0, lib.pt_last_error(c)
            assert host_pass() == 0, lib.pt_last_error(c)
            for k in (1, 3, 5, 7):  # oldest render first
                assert steps[k]() == 0, lib.pt_last_error(c)
        else:
            for s in steps:
                assert s() in (None, 0), lib.pt_last_error(c)
            assert host_pass() == 0, lib.pt_last_error(c)
        out = {}
        for name, ptr, arr in (("img", d_img, np.zeros((h, w, 3), dtype=np.uint8)), ("img2", d_img2, np.zeros((h, w, 3), dtype=np.uint8)), ("depth", d_depth, np.zeros((h, w))),
                               ("node", d_node, np.zeros((h, w), dtype=np.int32)), ("t", d_t, np.zeros(n)), ("id", d_id, np.zeros(n, dtype=np.int32)),
                               ("rad", d_rad, np.zeros((n, 3)))):
            assert lib.pt_copy_from_device(c, arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
            out[name] = arr
        out["host_rad"] = host_rad
        for p in (d_bg, d_o, d_d, d_bgr, d_img, d_img2, d_depth, d_node, d_t, d_id, d_rad):
            lib.pt_device_free(c, p)
        ctx.close()
        results.append(out)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), k
    assert (results[1]["id"] >= 0).sum() > 1000 and results[1]["img"].any()
    # and the radiance pass is the oracle's render of the same (shuffled) pixel centres
    ref = oracle.render(oracle.pack(scene), cam0, w, h, background=bg, samples=1, seed=6, jitter=oracle.JITTER_CENTRE, mode=oracle.MODE_FLAT)
    same_bits(results[1]["rad"], ref.linear.reshape(-1, 3)[order], "radiance in flight vs po_render")


def test_argument_errors(host, H):
    lib = H.lib()
    sc = host.Scene.example("primitives", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ctx = r.context
    n = 100
    o, d, bg, rgb = np.zeros((n, 3)), np.ones((n, 3)), np.zeros(3), np.full((n, 3), 3.0)
    dp = lambda a: a.ctypes.data_as(H._dp)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    good = H.PtRadianceParams(n, 0, 0, 0, 0, 0)
    for fn, cv in ((lib.pt_radiance, dp), (lib.pt_radiance_device, vp)):
        assert fn(ctx, None, cv(o), cv(d), cv(bg), cv(rgb), None) == H.ERR_ARGUMENT
        for hole in range(4):
            a = [cv(o), cv(d), cv(bg), cv(rgb)]
            a[hole] = None
            assert fn(ctx, C.byref(good), *a, None) == H.ERR_ARGUMENT, hole
        assert fn(ctx, C.byref(H.PtRadianceParams(H.RAYS_MAX + 1, 0, 0, 0, 0, 0)), cv(o), cv(d), cv(bg), cv(rgb), None) == H.ERR_ARGUMENT
        for ro, pr in ((2, 0), (-1, 0), (0, 2), (0, -1)):
            assert fn(ctx, C.byref(H.PtRadianceParams(n, ro, pr, 0, 0, 0)), cv(o), cv(d), cv(bg), cv(rgb), None) == H.ERR_ARGUMENT, (ro, pr)
        assert fn(ctx, C.byref(H.PtRadianceParams(0, 0, 0, 0, 0, 0)), cv(o), cv(d), cv(bg), cv(rgb), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(rgb == 3.0)
    assert lib.pt_radiance_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    assert lib.pt_radiance(ctx, C.byref(good), dp(o), dp(d), dp(bg), dp(rgb), None) == H.OK
    bare = H.Context()
    assert lib.pt_radiance(bare.handle, C.byref(good), dp(o), dp(d), dp(bg), dp(rgb), None) == H.ERR_NO_SCENE
    assert lib.pt_radiance_device(bare.handle, C.byref(good), vp(o), vp(d), vp(bg), vp(rgb), None) == H.ERR_NO_SCENE
    assert lib.pt_radiance(bare.handle, C.byref(H.PtRadianceParams(n, 3, 0, 0, 0, 0)), dp(o), dp(d), dp(bg), dp(rgb), None) == H.ERR_ARGUMENT  # the argument comes first
    bare.close()
    empty = r.radiance(np.zeros((0, 3)), np.zeros((0, 3)))
    assert empty["rgb"].shape == (0, 3) and empty["kernel_ms"] == 0.0
    into = np.full((n, 3), -7.25)
    back = r.radiance(o + 50.0, d, background=(0.5, 0.25, 0.125), into=into)
    assert back["rgb"] is into and not np.any(into == -7.25)
    r.close()


# ---- the recursion frames all in HBM (PARK = 0 instantiations on a scene that parks frames)
@pytest.mark.parametrize("name", ["entering-the-mirror-dimension", "transmission-refraction"])
def test_recursion_frames_all_in_hbm(oracle, host, H, monkeypatch, name):
    """PORTRAYER_PARK=0, as for a render (tests/test_gpu_textures.py: the test of this name): no parked frame stays in LDS, every push and pop goes through the
    lane's HBM lines. Same bits as with the youngest frame in LDS, and as the oracle."""
    scene, cam, _ = all_examples()[name]()
    ps = oracle.pack(scene)
    hs = host_glue.host_scene(scene)
    o, d = pixel_centre_rays(oracle, cam, W, HT)
    order = np.random.default_rng(8).permutation(len(o))
    o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(hs, tr, kd_depth=8)
        in_lds = r.radiance(o, d, background=BG, seed=0)["rgb"]
        monkeypatch.setenv("PORTRAYER_PARK", "0")
        in_hbm = [r.radiance(o, d, background=BG, seed=0, reorder=ro)["rgb"] for ro in (False, True)]
        monkeypatch.delenv("PORTRAYER_PARK")
        r.close()
        same_bits(in_hbm[0], in_lds, f"{name} {mname}: frames in HBM vs youngest in LDS")
        same_bits(in_hbm[1], in_hbm[0], f"{name} {mname}: frames in HBM, reorder")
        same_bits(in_hbm[0], oracle_color(oracle, ps, o, d, om, 8), f"{name} {mname}: frames in HBM vs po_color_rays")
