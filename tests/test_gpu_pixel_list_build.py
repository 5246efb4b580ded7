"""How the list kernel builds the per-pixel candidate lists (pt_api.hip: pt_pixel_list_kernel): it opens the scene tree up to 64 nodes at a time with the
beam of the whole 8x8 tile, keeps the pending inner nodes and the leaves found in per-wavefront LDS buffers, and flushes the leaves in batches through every lane's own
pixel beam. The cases here push on those buffers and on the tile's rectangle; tests/test_gpu_pixel_lists.py holds the lists' cases proper. In every case the image and
the f64 means are the oracle's, bit for bit, and the launch's raw records (pt_test_pixel_list_records) are well formed:

  the count is at most the cap; the entries are strictly ascending as words; the node indices are below the scene's node count and distinct; a finite tail is not below
  the last entry's bound (and only a full list has one); the words behind the last entry are zero; a tile's 64 records are marked "take the walk" together or not at all.

(a) the whole of big-scene in one tile (8x8) and in two (16x8): the pending list runs hundreds deep and the candidates are flushed many times; nothing is marked.
(b) a generated scene of 3,000 small primitives seen by one 8x8 tile: each tile wholly marked or not at all, the image the oracle's either way. The kernel pops the
    pending list from its end, so a balanced tree of n leaves leaves about 64 log2(n / 64) nodes pending at most, and a scene of this size does not fill the 1,024
    words: the marked tiles are reached with PORTRAYER_PIXEL_LIST_PENDING (tests only), which shrinks the list - to 300, 64 and 1 node.
(c) a 9x7 image and a two-rank partition of 24x16: slots outside the slice, and tiles of the other rank, inside a tile's rectangle."""
import ctypes as C

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cube, Light, Material, Node, Scene, Sphere, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

WALK = 0x80000000
INF_BITS = 0x7F800000
KEYS = ("PORTRAYER_PIXEL_LISTS", "PORTRAYER_PIXEL_LIST_CAP", "PORTRAYER_PIXEL_LIST_PENDING")


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def big(host, oracle):
    from example_scenes import EXAMPLES
    from scene_dsl import ASSETS
    sc = host.Scene.example("big-scene", assets=ASSETS)
    packed = oracle.pack_arrays(sc.export())
    cam = EXAMPLES["big-scene"]()[1]
    refs = {}

    def ref(w, h, samples, seed):
        key = (w, h, samples, seed)
        if key not in refs:
            refs[key] = oracle.render(packed, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        return refs[key]
    return sc, ref


def flat_kernel(H, st):
    return st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER | H.KERNEL_COUNTING)


def records(H, context):
    """The last launch's raw records as (records, words) uint32, the entries a record holds at most, the scene's node count."""
    info = (C.c_uint64 * 4)()
    assert H.lib().pt_test_pixel_list_records(context, None, 0, info) == 0, H.lib().pt_last_error(context)
    n, words, k, n_nodes = (int(v) for v in info)
    assert n > 0 and n % 64 == 0 and words >= 2 + k
    rec = np.zeros((n, words), np.uint32)
    assert H.lib().pt_test_pixel_list_records(context, rec.ctypes.data_as(C.POINTER(C.c_uint32)), rec.size, info) == 0, H.lib().pt_last_error(context)
    assert int(info[0]) == n
    return rec, k, n_nodes


def check_records(rec, k, n_nodes, cap=None):
    """The structural checks of the module's head. Returns the number of marked tiles and the longest list."""
    cap = k if cap is None else cap
    n = len(rec)
    head, tail, ent = rec[:, 0], rec[:, 1], rec[:, 2:2 + k].astype(np.int64)
    marked = (head & WALK) != 0
    tiles = marked.reshape(n // 64, 64)
    assert np.all(tiles.all(axis=1) | ~tiles.any(axis=1)), "a tile is marked in part"
    ok = ~marked
    count = (head & 0xFF).astype(np.int64)
    assert np.all(head[ok] == count[ok]) and np.all(count[ok] <= cap), (count[ok].max(), cap)
    col = np.arange(k)[None, :]
    used = ok[:, None] & (col < count[:, None])
    assert np.all(ent[ok[:, None] & ~used] == 0) and np.all(rec[ok, 2 + k:] == 0)
    pair = used[:, 1:]  # entry j + 1 is in use: so is entry j
    assert np.all(ent[:, 1:][pair] > ent[:, :-1][pair]), "entries not strictly ascending"
    node = ent & 0xFFFF
    assert np.all(node[used] < n_nodes)
    srt = np.sort(np.where(used, node, -1 - col), axis=1)  # (unused columns get distinct negatives)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "a node twice in a list"
    bound = (ent & 0xFFFF0000).astype(np.uint32).view(np.float32)
    assert np.all(np.isfinite(bound[used])) and np.all(bound[used] >= 0.0)
    finite = ok & (tail != INF_BITS)
    t = tail.view(np.float32)
    assert np.all(np.isfinite(t[finite])) and np.all(t[finite] >= 0.0) and np.all(count[finite] == cap), "a tail that is no bound, or one on a list with room left"
    if cap > 0:
        last = bound[np.arange(n), np.maximum(count - 1, 0)]
        assert np.all(t[finite] >= last[finite]), "a tail below the last entry's bound"
    return int(tiles.all(axis=1).sum()), int(count[ok].max()) if ok.any() else 0


def render_and_check(H, r, cam10, ref, w, h, samples, seed, cap=None):
    rgb, lin, st = r.render(cam10, w, h, default_background(w, h), samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG)
    assert flat_kernel(H, st), st
    assert np.array_equal(rgb, ref.rgb), f"{(rgb != ref.rgb).any(axis=2).sum()} pixels differ from the oracle"
    assert_ulp(lin, ref.linear, 0, "f64 means")
    rec, k, n_nodes = records(H, r.context)
    assert len(rec) == ((w + 7) // 8) * ((h + 7) // 8) * 64
    return rec, check_records(rec, k, n_nodes, cap)


# ---- (a) the whole scene in one tile

@pytest.mark.parametrize("w,h", [(8, 8), (16, 8)], ids=["one tile", "two tiles"])
def test_big_scene_in_one_or_two_tiles(host, H, big, w, h):
    sc, ref = big
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    try:
        rf = ref(w, h, 64, 3)
        assert rf.stats["hits"] > 0
        rec, (marked, longest) = render_and_check(H, r, sc.camera, rf, w, h, 64, 3)
        assert marked == 0
        assert longest == 6 and np.any(rec[:, 1] != INF_BITS)  # pixels this large reach more leaves than a record holds: lists cut at the shipped K
    finally:
        r.close()


# ---- (b) a pending list that runs full

def many_small_primitives(n=3000):
    """n small spheres and cubes on a jittered 60-column grid in front of the camera, all of them inside an 8x8 image's view."""
    rng = np.random.default_rng(11)
    m = [Material(diffuse=(0.8, 0.3, 0.2), specular=(0.5, 0.5, 0.5), shininess=25.0), Material(diffuse=(0.2, 0.7, 0.3), specular=(0.0, 0.0, 0.0)),
         Material(diffuse=(0.3, 0.4, 0.8), specular=(0.6, 0.6, 0.3), shininess=300.0)]
    kids = []
    for i in range(n):
        gx, gy = i % 60, i // 60
        pos = (-3.0 + 0.1 * gx + 0.03 * rng.random(), -2.5 + 0.1 * gy + 0.03 * rng.random(), -1.0 + 2.0 * rng.random())
        kids.append(Node.geo(Sphere() if i % 3 else Cube(), m[i % 3]).scaled(0.02 + 0.03 * rng.random()).translated(pos))
    lights = [Light(position=(3.0, 8.0, 6.0), color=(0.8, 0.8, 0.8)), Light(position=(-5.0, 2.0, 7.0), color=(0.3, 0.3, 0.4))]
    return Scene(root=Node.group(kids), lights=lights, ambient=(0.1, 0.1, 0.1)), Camera(eye=(0.0, 0.0, 9.0), center=(0.0, 0.0, 0.0), fovy_degrees=50.0)


@pytest.fixture(scope="module")
def crowd(host, oracle):
    scene, cam = many_small_primitives()
    refs = {}

    def ref(w, h):
        if (w, h) not in refs:
            refs[(w, h)] = oracle.render(scene, cam, w, h, samples=64, seed=9, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        return refs[(w, h)]
    return host_glue.host_scene(scene), host_glue.cam10(cam), ref


@pytest.mark.parametrize("pending", [None, 300, 64, 1], ids=["the shipped capacity", "300 nodes", "64 nodes", "1 node"])
@pytest.mark.parametrize("w,h", [(8, 8), (16, 8)], ids=["one tile", "two tiles"])
def test_three_thousand_primitives_in_a_tile(host, H, crowd, monkeypatch, w, h, pending):
    hs, cam10, ref = crowd
    rf = ref(w, h)
    assert rf.stats["hits"] > 0
    if pending is not None:
        monkeypatch.setenv("PORTRAYER_PIXEL_LIST_PENDING", str(pending))
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    try:
        rec, (marked, longest) = render_and_check(H, r, cam10, rf, w, h, 64, 9)
        tiles = len(rec) // 64
        # (every tile sees hundreds of primitives: the root's two children are inner nodes within its beam, so one pending word cannot hold them, and 64 words run out
        # once a step of 64 nodes leaves more than 64 inner children)
        if pending in (64, 1):
            assert marked == tiles, (pending, marked, tiles)
        if marked < tiles:
            assert longest == 6
    finally:
        r.close()


def test_the_pending_capacity_is_checked(host, H, crowd, monkeypatch):
    hs, cam10, ref = crowd
    r = host.Renderer(hs, H.TRAVERSE_FLAT)
    try:
        for bad in ("0", "1025", "x"):
            monkeypatch.setenv("PORTRAYER_PIXEL_LIST_PENDING", bad)
            with pytest.raises(host.PortrayerHostError):
                r.render(cam10, 8, 8, default_background(8, 8), samples=64, seed=9, sample_mode=H.SAMPLE_RNG)
    finally:
        r.close()


# ---- (c) partial tiles and a rank partition

def test_partial_tiles(host, H, big):
    """9x7: two tiles, both partial - most slots of the second lie outside the image, and the tile's rectangle reaches past both edges."""
    sc, ref = big
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    try:
        rec, (marked, longest) = render_and_check(H, r, sc.camera, ref(9, 7, 64, 3), 9, 7, 64, 3)
        assert marked == 0 and len(rec) == 128
    finally:
        r.close()


def test_two_rank_partition(host, H, big):
    """24x16 = six tiles, rank 0 of 2 then rank 1 of 2 into the same buffers: a launch's records are its own three tiles', each opened with its own rectangle."""
    sc, ref = big
    w, h, samples, seed = 24, 16, 64, 3
    rf = ref(w, h, samples, seed)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(w, h))
    cam = host.camera(sc.camera, w, h)
    dp = C.POINTER(C.c_double)
    try:
        rgb = np.zeros((h, w, 3), np.uint8)
        lin = np.zeros((h, w, 3), np.float64)
        per_rank = []
        for rank in (0, 1):
            p = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, seed, H.SAMPLE_RNG, 1 if bg.shape == (h, 3) else 0, rank, 2, 0)
            st = H.PtStats()
            assert lib.pt_render(c, C.byref(cam), bg.ctypes.data_as(dp), C.byref(p), rgb.ctypes.data_as(C.POINTER(C.c_uint8)), lin.ctypes.data_as(dp), C.byref(st)) == 0, lib.pt_last_error(c)
            assert flat_kernel(H, st.as_dict())
            rec, k, n_nodes = records(H, c)
            assert len(rec) == 3 * 64
            marked, _ = check_records(rec, k, n_nodes)
            assert marked == 0
            per_rank.append(rec.copy())
        assert not np.array_equal(per_rank[0], per_rank[1])  # other tiles, other lists
        assert np.array_equal(rgb, rf.rgb), f"{(rgb != rf.rgb).any(axis=2).sum()} pixels differ from the oracle"
        assert_ulp(lin, rf.linear, 0, "f64 means")
    finally:
        r.close()
