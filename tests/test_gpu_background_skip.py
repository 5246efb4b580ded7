"""The queue of the pixels that need the render kernel (pt_pixel_list.h: PT_PL_QUEUE; pt_api.hip: pt_pixel_list_kernel, pt_finish_kernel; pt_render_simple.h).
A pixel whose candidate list is empty with nothing left out is background for every sample: the list kernel leaves it out of the queue, the render kernel is dealt only
what is queued, and the finish kernel gives such a pixel the sum of its background samples (pt_background_sum) without any chunk sum having been written. Every image and
every f64 mean must stay the oracle's, bit for bit, by three routes: the default, PORTRAYER_BACKGROUND_SKIP=0 (the lists, every item dealt) and PORTRAYER_PIXEL_LISTS=0
(the walk). After every default launch the queue itself is read back (pt_test_pixel_list_queue) and compared with the launch's records: it must hold exactly the slots
inside the slice whose record is not {0 entries, infinite tail, unmarked}, each once, a tile's together in the tile's Morton order, and the count must be its length."""
import ctypes as C

import numpy as np
import pytest

import host_glue
from scene_dsl import Camera, Cone, Cube, Cylinder, Light, Material, Node, Scene, Sphere, default_background
from ulp import assert_ulp

pytestmark = pytest.mark.gpu

WALK = 0x80000000
INF_BITS = 0x7F800000
ROUTES = [("default", {}), ("every item dealt", {"PORTRAYER_BACKGROUND_SKIP": "0"}), ("walk", {"PORTRAYER_PIXEL_LISTS": "0"})]
KEYS = ("PORTRAYER_BACKGROUND_SKIP", "PORTRAYER_PIXEL_LISTS", "PORTRAYER_PIXEL_LIST_CAP", "PORTRAYER_PIXEL_LIST_PENDING", "PORTRAYER_FINE_QUEUES")
W, HGT = 24, 16


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


def routes(monkeypatch, extra=None):
    """Yields each route's name with its environment set (extra: what the case itself sets, on every route)."""
    for name, env in ROUTES:
        for k in KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in {**(extra or {}), **env}.items():
            monkeypatch.setenv(k, v)
        yield name


def flat_kernel(H, st):
    return st["kernel_mode"] == 3 and not st["kernel_variant"] & (H.KERNEL_CHAIN | H.KERNEL_INTERPRETER | H.KERNEL_COUNTING)


# ---- the queue against the records

MORTON = [((q & 1) | ((q >> 1) & 2) | ((q >> 2) & 4)) + 8 * (((q >> 1) & 1) | ((q >> 2) & 2) | ((q >> 3) & 4)) for q in range(64)]  # pt_tile_order_to_slot


def records(H, context):
    info = (C.c_uint64 * 4)()
    assert H.lib().pt_test_pixel_list_records(context, None, 0, info) == 0, H.lib().pt_last_error(context)
    n, words = int(info[0]), int(info[1])
    rec = np.zeros((n, words), np.uint32)
    if n:
        assert H.lib().pt_test_pixel_list_records(context, rec.ctypes.data_as(C.POINTER(C.c_uint32)), rec.size, info) == 0, H.lib().pt_last_error(context)
    return rec


def queue(H, context):
    """(the launch had a queue, its ids in the order the device left them, the launch's slots)"""
    info = (C.c_uint64 * 3)()
    assert H.lib().pt_test_pixel_list_queue(context, None, 0, info) == 0, H.lib().pt_last_error(context)
    has, count, slots = int(info[0]), int(info[1]), int(info[2])
    ids = np.zeros(max(count, 1), np.uint32)
    assert H.lib().pt_test_pixel_list_queue(context, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, info) == 0, H.lib().pt_last_error(context)
    assert int(info[1]) == count
    return bool(has), ids[:count], slots


def inside_slice(n_slots, rect, rank=0, ranks=1):
    """pt_slot_to_pixel: which slots of the launch lie inside the slice."""
    x0, y0, x1, y1 = rect
    tiles_x = (x1 - x0 + 1 + 7) // 8
    p = np.arange(n_slots)
    tile, j = (p >> 6) * ranks + rank, p & 63
    px, py = x0 + (tile % tiles_x) * 8 + (j & 7), y0 + (tile // tiles_x) * 8 + (j >> 3)
    return (px <= x1) & (py <= y1)


def check_queue(name, H, context, rect, rank=0, ranks=1):
    """After a launch by route `name`. Returns the queued pixels per tile of the launch (None: no queue)."""
    has, ids, slots = queue(H, context)
    if name != "default":
        assert not has and len(ids) == 0, (name, has, len(ids))
        return None
    assert has, "the default launch had no queue"
    rec = records(H, context)
    assert len(rec) == slots and slots % 64 == 0
    background = (rec[:, 0] == 0) & (rec[:, 1] == INF_BITS)
    want = np.flatnonzero(inside_slice(slots, rect, rank, ranks) & ~background)
    assert len(ids) == len(want), (len(ids), len(want))  # the count is the queue's length ...
    assert np.array_equal(np.sort(ids), want), "the queue does not hold exactly the pixels that need the kernel"  # ... and each of them is there once
    if len(ids) == 0:
        return np.zeros(slots // 64, np.int64)
    # a tile's ids lie together, in the tile's Morton order
    tiles = ids >> 6
    starts = np.flatnonzero(np.r_[True, tiles[1:] != tiles[:-1]])
    assert np.all(np.diff(tiles[starts].astype(np.int64)) > 0), "the tiles' ranges are not in the order of the tiles"  # (so each tile has one run)
    order = np.argsort(MORTON)  # j -> its place in the Morton order
    place = order[ids & 63]
    same = tiles[1:] == tiles[:-1]
    assert np.all(place[1:][same] > place[:-1][same]), "a tile's ids out of Morton order"
    return np.bincount(want >> 6, minlength=slots // 64)


# ---- scenes

def lights():
    return [Light(position=(3.0, 8.0, 6.0), color=(0.7, 0.7, 0.7)), Light(position=(-5.0, 6.0, 4.0), color=(0.3, 0.3, 0.4), falloff=(1.0, 0.01, 0.001))]


def materials():
    return [Material(diffuse=(0.8, 0.3, 0.2), specular=(0.5, 0.5, 0.5), shininess=25.0), Material(diffuse=(0.2, 0.7, 0.3), specular=(0.0, 0.0, 0.0)),
            Material(diffuse=(0.3, 0.4, 0.8), specular=(0.6, 0.6, 0.3), shininess=300.0)]


def small_sphere():
    """A sphere whose box projects onto columns 8 .. 17 and rows 0 .. 7 of the 24x16 frame of CAM (and a small one in front of it, so that the tree has a root to test):
    the tile of columns 8 .. 15 is covered, the one right of it in part, the other four not at all."""
    m = materials()
    kids = [Node.geo(Sphere(), m[0]).scaled(1.603).translated((0.28, 1.827, 0.0)), Node.geo(Sphere(), m[2]).scaled(0.2).translated((0.28, 1.827, 1.7))]
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))


def filling_cube():
    m = materials()
    kids = [Node.geo(Cube(), m[1]).scaled((40.0, 40.0, 1.0)).rotated_z(0.1).translated((0.0, 0.0, -3.0)), Node.geo(Sphere(), m[0]).scaled(0.5).translated((0.3, 0.2, 1.0))]
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))


def scattered():
    """Eight primitives across the frame: a tree with inner nodes below the root, background between them."""
    m = materials()
    kids = [Node.geo(p(), m[k % 3]).scaled(0.45 + 0.05 * k).rotated_y(0.3 * k).translated((-3.2 + 0.9 * k, 1.4 - 0.8 * (k % 3), -0.5 * (k % 2)))
            for k, p in enumerate((Sphere, Cube, Cylinder, Cone, Sphere, Cube, Cylinder, Cone))]
    return Scene(root=Node.group(kids), lights=lights(), ambient=(0.1, 0.1, 0.1))


CAM = Camera(eye=(0.0, 0.0, 8.0), center=(0.0, 0.0, 0.0))
CAM_AWAY = Camera(eye=(0.0, 0.0, 8.0), center=(0.0, 0.0, 16.0))


@pytest.fixture(scope="module")
def sphere_ref(oracle):
    """The oracle's renders of the small-sphere scene, each computed once."""
    scene, refs = small_sphere(), {}

    def ref(w=W, h=HGT, samples=64, seed=5, cam=CAM):
        key = (w, h, samples, seed, id(cam))
        if key not in refs:
            refs[key] = oracle.render(scene, cam, w, h, samples=samples, seed=seed, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
        return refs[key]
    return scene, ref


def run(monkeypatch, H, host, scene, cam, ref, w=W, h=HGT, samples=64, seed=5, rect=None, background=None, extra=None):
    """The three routes against the oracle's image and f64 means; the queue after each. Returns the default route's queued pixels per tile."""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, w - 1, h - 1)
    bg = default_background(w, h) if background is None else background
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    per_tile = None
    try:
        for name in routes(monkeypatch, extra):
            into = np.full((h, w, 3), 7, np.uint8)
            rgb, lin, st = r.render(host_glue.cam10(cam), w, h, bg, samples=samples, seed=seed, sample_mode=H.SAMPLE_RNG, rect=rect, into=into)
            assert flat_kernel(H, st), (name, st)
            a, b = rgb[y0:y1 + 1, x0:x1 + 1], ref.rgb[y0:y1 + 1, x0:x1 + 1]
            assert np.array_equal(a, b), f"{name}: {(a != b).any(axis=2).sum()} pixels differ from the oracle"
            assert_ulp(lin[y0:y1 + 1, x0:x1 + 1], ref.linear[y0:y1 + 1, x0:x1 + 1], 0, name)
            outside = np.ones((h, w), bool)
            outside[y0:y1 + 1, x0:x1 + 1] = False
            assert (rgb[outside] == 7).all(), f"{name}: bytes outside the slice changed"
            q = check_queue(name, H, r.context, (x0, y0, x1, y1))
            if name == "default":
                per_tile = q
    finally:
        r.close()
    return per_tile


# ---- the cases

def test_mixed_tiles(monkeypatch, H, host, sphere_ref):
    scene, ref = sphere_ref
    rf = ref()
    assert 0 < rf.stats["hits"] < rf.stats["primary"]
    per_tile = run(monkeypatch, H, host, scene, CAM, rf)
    assert (per_tile == 0).any() and (per_tile == 64).any() and ((per_tile > 0) & (per_tile < 64)).any(), per_tile  # wholly background, not at all, partly


def test_count_zero(monkeypatch, H, host, sphere_ref):
    """The camera turned away: nothing is queued, and the render kernel runs with zero items."""
    scene, ref = sphere_ref
    rf = ref(cam=CAM_AWAY)
    assert rf.stats["hits"] == 0
    per_tile = run(monkeypatch, H, host, scene, CAM_AWAY, rf)
    assert per_tile.sum() == 0


def test_nothing_skipped(monkeypatch, H, host, oracle):
    scene = filling_cube()
    rf = oracle.render(scene, CAM, W, HGT, samples=64, seed=5, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert rf.stats["hits"] == rf.stats["primary"]
    per_tile = run(monkeypatch, H, host, scene, CAM, rf)
    assert per_tile.sum() == W * HGT


def test_partial_tiles(monkeypatch, H, host, sphere_ref):
    """9x7: two tiles, both partial - the slots outside the image are never queued, whatever their records say."""
    scene, ref = sphere_ref
    per_tile = run(monkeypatch, H, host, scene, CAM, ref(9, 7), w=9, h=7)
    assert len(per_tile) == 2 and per_tile.sum() <= 63


def test_a_slice_off_the_tile_grid(monkeypatch, H, host, sphere_ref):
    scene, ref = sphere_ref
    per_tile = run(monkeypatch, H, host, scene, CAM, ref(), rect=(5, 1, 20, 13))
    assert len(per_tile) == 4 and 0 < per_tile.sum() < 16 * 13


@pytest.mark.parametrize("samples", [57, 60, 121, 128], ids=["a last chunk of 1", "a last chunk of 4", "two groups, a last chunk of 1", "two groups"])
def test_sample_counts(monkeypatch, H, host, sphere_ref, samples):
    scene, ref = sphere_ref
    per_tile = run(monkeypatch, H, host, scene, CAM, ref(samples=samples), samples=samples)
    assert 0 < per_tile.sum() < W * HGT


def test_a_background_colour_per_pixel(monkeypatch, H, host, oracle):
    """background_rows = 0: a different colour in every pixel, -0.0 and 0.1 among them; the f64 means are compared bit for bit."""
    rng = np.random.default_rng(7)
    bg = rng.random((HGT, W, 3))
    bg[0, 0] = (-0.0, 0.1, -0.0)
    bg[HGT - 1, W - 1] = (0.1, -0.0, 0.1)
    bg[9, 2] = (0.1, 0.1, 0.1)
    scene = small_sphere()
    rf = oracle.render(scene, CAM, W, HGT, background=bg, samples=64, seed=5, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert rf.stats["hits"] > 0
    per_tile = run(monkeypatch, H, host, scene, CAM, rf, background=bg)
    assert (per_tile == 0).any()


def test_a_cap_of_zero_entries(monkeypatch, H, host, sphere_ref):
    """PORTRAYER_PIXEL_LIST_CAP=0: every list is empty, but the tail is finite wherever a leaf was reached - those pixels need the kernel and must be queued."""
    scene, ref = sphere_ref
    plain = run(monkeypatch, H, host, scene, CAM, ref())
    capped = run(monkeypatch, H, host, scene, CAM, ref(), extra={"PORTRAYER_PIXEL_LIST_CAP": "0"})
    assert np.array_equal(plain, capped) and capped.sum() > 0


def test_marked_tiles(monkeypatch, H, host, oracle):
    """PORTRAYER_PIXEL_LIST_PENDING=1: tiles whose pending list runs full are marked "take the walk", and every in-slice slot of a marked tile is queued."""
    scene = scattered()
    rf = oracle.render(scene, CAM, W, HGT, samples=64, seed=5, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT)
    assert 0 < rf.stats["hits"] < rf.stats["primary"]
    plain = run(monkeypatch, H, host, scene, CAM, rf)
    marked = run(monkeypatch, H, host, scene, CAM, rf, extra={"PORTRAYER_PIXEL_LIST_PENDING": "1"})
    assert (marked == 64).any() and marked.sum() > plain.sum(), (plain, marked)  # (a marked tile is queued whole: more than the lists alone ask for)


def test_guided_batches(monkeypatch, H, host, sphere_ref):
    """PORTRAYER_FINE_QUEUES=0: the hand-out of very long launches - batches from one counter - over the queue."""
    scene, ref = sphere_ref
    per_tile = run(monkeypatch, H, host, scene, CAM, ref(), extra={"PORTRAYER_FINE_QUEUES": "0"})
    assert 0 < per_tile.sum() < W * HGT


def test_two_rank_partition(monkeypatch, H, host, sphere_ref):
    """24x16 = six tiles, compact = 1: each rank's buffer rendered here, its queue its own three tiles', then untiled on the device."""
    scene, ref = sphere_ref
    rf = ref()
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    lib, ctx = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(W, HGT))
    cam = host.camera(host_glue.cam10(CAM), W, HGT)
    d_bg, d_gath, d_full = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rect = (0, 0, W - 1, HGT - 1)
    try:
        p0 = H.PtRenderParams(W, HGT, H.PtRect(*rect), 64, 5, H.SAMPLE_RNG, 1, 0, 2, 0)
        per = int(lib.pt_compact_bytes(C.byref(p0)))
        assert lib.pt_device_alloc(ctx, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(ctx, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        assert lib.pt_device_alloc(ctx, per * 2, C.byref(d_gath)) == 0 and lib.pt_device_alloc(ctx, W * HGT * 3, C.byref(d_full)) == 0
        for name in routes(monkeypatch):
            queued = 0
            for rank in (0, 1):
                p = H.PtRenderParams(W, HGT, H.PtRect(*rect), 64, 5, H.SAMPLE_RNG, 1, rank, 2, 0)
                st = H.PtStats()
                assert lib.pt_render_device(ctx, C.byref(cam), d_bg, C.byref(p), 1, C.c_void_p(d_gath.value + rank * per), None) == 0, lib.pt_last_error(ctx)
                assert lib.pt_render_finish(ctx, C.byref(st)) == 0, lib.pt_last_error(ctx)
                assert flat_kernel(H, st.as_dict())
                q = check_queue(name, H, ctx, rect, rank, 2)
                if q is not None:
                    assert len(q) == 3
                    queued += int(q.sum())
            if name == "default":
                assert 0 < queued < W * HGT
            assert lib.pt_untile_device(ctx, C.byref(p0), d_gath, d_full, None) == 0 and lib.pt_synchronize(ctx) == 0, lib.pt_last_error(ctx)
            img = np.zeros((HGT, W, 3), np.uint8)
            assert lib.pt_copy_from_device(ctx, img.ctypes.data_as(C.c_void_p), d_full, img.nbytes) == 0
            assert np.array_equal(img, rf.rgb), f"{name}: {(img != rf.rgb).any(axis=2).sum()} pixels differ from the oracle"
    finally:
        for d in (d_bg, d_gath, d_full):
            if d:
                lib.pt_device_free(ctx, d)
        r.close()


def test_two_frames_in_flight(monkeypatch, H, host, sphere_ref):
    """pt_render_device on the context's two streams, both open at once, with different cameras: a slot's queue and count are its own frame's."""
    scene, ref = sphere_ref
    cams = [CAM, CAM_AWAY, Camera(eye=(1.5, 0.5, 8.0), center=(0.0, 0.5, 0.0))]
    refs = [ref(seed=20 + k, cam=cam) for k, cam in enumerate(cams)]
    assert not np.array_equal(refs[0].rgb, refs[2].rgb)
    r = host.Renderer(host_glue.host_scene(scene), H.TRAVERSE_FLAT)
    lib, c = H.lib(), r.context
    bg = np.ascontiguousarray(default_background(W, HGT))
    d_bg, d_img = C.c_void_p(), [C.c_void_p(), C.c_void_p()]
    try:
        assert lib.pt_device_alloc(c, bg.nbytes, C.byref(d_bg)) == 0 and lib.pt_copy_to_device(c, d_bg, bg.ctypes.data_as(C.c_void_p), bg.nbytes) == 0
        for d in d_img:
            assert lib.pt_device_alloc(c, W * HGT * 3, C.byref(d)) == 0
        for name in routes(monkeypatch):
            st, got, slots = H.PtStats(), [], []

            def close(k):
                assert lib.pt_render_finish(c, C.byref(st)) == 0, lib.pt_last_error(c)
                img = np.zeros((HGT, W, 3), dtype=np.uint8)
                assert lib.pt_copy_from_device(c, img.ctypes.data_as(C.c_void_p), d_img[slots[k]], img.nbytes) == 0
                got.append((img, st.as_dict()))

            for k, cam in enumerate(cams):
                slot = int(lib.pt_context_next_slot(c))
                slots.append(slot)
                p = H.PtRenderParams(W, HGT, H.PtRect(0, 0, W - 1, HGT - 1), 64, 20 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
                camera = host.camera(host_glue.cam10(cam), W, HGT)
                assert lib.pt_render_device(c, C.byref(camera), d_bg, C.byref(p), 0, d_img[slot], C.c_void_p(lib.pt_context_stream(c, slot))) == 0, lib.pt_last_error(c)
                if k > 0:
                    close(k - 1)
            close(len(cams) - 1)
            assert slots[0] != slots[1]
            q = check_queue(name, H, c, (0, 0, W - 1, HGT - 1))  # (the last frame's)
            if q is not None:
                assert q.sum() > 0
            for k, ((img, stk), rf) in enumerate(zip(got, refs)):
                assert flat_kernel(H, stk), stk
                assert np.array_equal(img, rf.rgb), f"{name}, frame {k}: {(img != rf.rgb).any(axis=2).sum()} pixels differ from its own camera's image"
    finally:
        for d in d_img + [d_bg]:
            if d:
                lib.pt_device_free(c, d)
        r.close()
