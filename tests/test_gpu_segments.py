"""Ray queries over bounded segments (pt_segments / pt_segments_device / Renderer.rays(t_max=)) against the unchanged oracle, bit for bit.

The expectation is the FILTERED oracle: po_cast_rays gives t_o, and a ray hits inside its bound iff t_o < t_max; what it hits is then what po_cast_rays
reports, everything else is a miss. Every comparison is exact (bits() equality for f64, array equality for integers) and no ray is left out. The oracle
answers for t, the flat node, the point and the normal; `sub`, `material` and the hierarchical `node` are compared exactly with the unbounded pass on the same
rays (which tests/test_gpu_rays.py ties to the oracle), filtered the same way.

The batches are test_gpu_rays.incoherent_batch's (octants mixed in nearly every wavefront), thinned so that about three quarters of the rays hit something,
since a ray that hits nothing says nothing about a bound. The bounds, per ray and per traversal (t_o differs between the semantics), in shares 2 : 1 : 1 : 1 : 1 : 1
(the issue's list - a third and five sixths - scaled to a whole): t_o times a factor in [0.25, 4]; exactly t_o (a miss: the range is half-open);
nextafter(t_o, inf) (a hit); +inf; an empty range (0, -0, negative, PT_EPSILON itself, below it, -inf, NaN); a random length."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scene_dsl import ASSETS, default_background  # noqa: E402
from test_gpu_aov import bits, compare, modes, packed_tri_off  # noqa: E402
from test_gpu_rays import ALL, as_aov, flat_of, incoherent_batch, load_scene, oracle_rays, same, scene_box  # noqa: E402

pytestmark = pytest.mark.gpu

N = 20_000
EPSILON = 1e-5  # PT_EPSILON (csrc/pt_math.h, math.rs:15)
EMPTY = np.array([0.0, -0.0, -1.0, EPSILON, EPSILON / 2, -np.inf, np.nan, -1e300])
# big-scene: mesh-free, 1000 nodes; macho-cows: plain meshes; robot-alarm-clock: KDMesh trees; instance: groups inside rotated groups inside a rotated root
SCENES = {"big-scene": {"flat": 3, "kd": 7, "hier": 6}, "macho-cows": {"flat": 1, "kd": 9, "hier": 8}, "robot-alarm-clock": {"flat": 4, "kd": 2, "hier": 5},
          "instance": {"flat": 1, "kd": 9, "hier": 8}}  # the kernel mode (PT_MODE_*) each traversal of the scene runs: all nine occur


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


def thinned_batch(O, ps, flat, seed, n=N):
    """n rays of a larger incoherent batch, in its order: three quarters of them hits (flat_scene), the rest misses. The larger batch is 2 n rays, doubled
    until it holds that many hits (open scenes: most rays of an incoherent batch meet nothing)."""
    for factor in (2, 4, 8, 16):
        o, d = incoherent_batch(O, ps, flat, seed, n=factor * n)
        t = oracle_rays(O, ps, o, d, O.MODE_FLAT, -1)["t"]
        hit, miss = np.flatnonzero(np.isfinite(t)), np.flatnonzero(~np.isfinite(t))
        if len(hit) >= (3 * n) // 4:
            break
    assert len(hit) >= (3 * n) // 4 and len(miss) >= n - (3 * n) // 4
    keep = np.sort(np.concatenate([hit[:(3 * n) // 4], miss[:n - (3 * n) // 4]]))
    return np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])


def bounds_for(rng, t_o, d, diag):
    """The mix of the module docstring for rays whose unbounded oracle answer is t_o (+inf: a miss, which takes a random length where t_o would be used)."""
    n = len(t_o)
    kind = rng.permutation(n) % 7
    length = diag / np.linalg.norm(d, axis=1) * 10.0 ** rng.uniform(-2.0, 0.5, size=n)
    base = np.where(np.isfinite(t_o), t_o, length)
    t_max = np.empty(n)
    k = kind <= 1
    t_max[k] = base[k] * 2.0 ** rng.uniform(-2.0, 2.0, size=int(k.sum()))
    t_max[kind == 2] = base[kind == 2]
    t_max[kind == 3] = np.nextafter(base[kind == 3], np.inf)
    t_max[kind == 4] = np.inf
    t_max[kind == 5] = EMPTY[rng.integers(0, len(EMPTY), size=int((kind == 5).sum()))]
    t_max[kind == 6] = length[kind == 6]
    waves = [len(np.unique(bits(t_max[i:i + 64]))) for i in range(0, n - 63, 64)]
    assert min(waves) > 32, "t_max must differ from lane to lane inside every wavefront"
    return t_max


def filtered(ref, t_max):
    """The oracle's answer restricted to [EPSILON, t_max): (expectation in oracle_rays' layout, which rays hit inside their bound)."""
    with np.errstate(invalid="ignore"):
        inside = (ref["id"] >= 0) & (ref["t"] < t_max)  # (false for a NaN bound; a bound <= EPSILON is below every t the oracle reports)
    out = dict(t=np.where(inside, ref["t"], np.inf), id=np.where(inside, ref["id"], -1).astype(np.int32), point=ref["point"].copy(), normal=ref["normal"].copy())
    out["point"][~inside] = 0.0
    out["normal"][~inside] = 0.0
    return out, inside


def filter_pass(base, inside):
    """The unbounded pass's buffers with the miss values wherever `inside` is false."""
    out = {}
    for k in ALL:
        miss = np.inf if k == "t" else (0 if k in ("position", "normal", "occluded") else -1)
        out[k] = np.where(inside.reshape((-1,) + (1,) * (base[k].ndim - 1)), base[k], np.asarray(miss, dtype=base[k].dtype))
    return out


def check(tag, got, exp, inside, base, flat, hier):
    """Every buffer of a nearest-hit segments pass, exactly: against the filtered oracle and against the filtered unbounded pass."""
    compare(tag, as_aov(got), exp, flat, hier=hier)
    assert np.array_equal(got["occluded"], inside.astype(np.uint8)), f"{tag}: occluded"
    same(got, filter_pass(base, inside))


_CASES = {}


def freeze(x):
    for a in (x.values() if isinstance(x, dict) else x):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, (dict, list)):
            freeze(a)


def case(O, host, H, which):
    """Scene, batch and per traversal the oracle's answers and the bounds made from them: computed once per scene, shared by the tests, never written to."""
    if which not in _CASES:
        sc, ps, tri_off, kd = load_scene(O, host, which)
        flat = flat_of(O, ps, tri_off)
        o, d = thinned_batch(O, ps, flat, seed=sum(map(ord, which)) + 1)
        lo, hi = scene_box(flat)
        rng = np.random.default_rng(len(which))
        per = {}
        for mname, _, om in modes(H, O):
            ref = oracle_rays(O, ps, o, d, om, kd)
            t_max = bounds_for(rng, ref["t"], d, float(np.linalg.norm(hi - lo)))
            exp, inside = filtered(ref, t_max)
            per[mname] = dict(ref=ref, t_max=t_max, exp=exp, inside=inside)
        freeze(per)
        freeze([o, d])
        _CASES[which] = dict(sc=sc, ps=ps, flat=flat, kd=kd, o=o, d=d, per=per)
    return _CASES[which]


def kernel_mode(r, sc):
    """The PT_MODE_* the context traces this scene with, as a render's statistics report it."""
    w, h = 16, 8
    return r.render(sc.camera, w, h, default_background(w, h), samples=1, stats=True)[2]["kernel_mode"]


# ---- 1. the filtered oracle, every traversal of every scene, both questions, both orders; and the unbounded limit
@pytest.mark.parametrize("which", list(SCENES))
def test_segments_match_the_filtered_oracle_in_every_traversal(oracle, host, H, which):
    c = case(oracle, host, H, which)
    o, d = c["o"], c["d"]
    for mname, tr, _ in modes(H, oracle):
        p = c["per"][mname]
        inside, cut = p["inside"], (p["ref"]["id"] >= 0) & ~p["inside"]
        print(f"{which} {mname}: {len(o)} rays, {int(inside.sum())} hit inside their bound, {int(cut.sum())} cut off by it")
        assert inside.sum() >= len(o) // 5 and cut.sum() >= len(o) // 5, "the batch must test the bound from both sides"
        r = host.Renderer(c["sc"], tr, kd_depth=c["kd"])
        assert kernel_mode(r, c["sc"]) == SCENES[which][mname]
        base = r.rays(o, d)
        base_occ = [r.rays(o, d, any_hit=True, reorder=ro)["occluded"] for ro in (False, True)]
        got = [r.rays(o, d, reorder=ro, t_max=p["t_max"]) for ro in (False, True)]
        occ = [r.rays(o, d, any_hit=True, reorder=ro, t_max=p["t_max"])["occluded"] for ro in (False, True)]
        unbounded = [r.rays(o, d, reorder=ro, t_max=np.inf) for ro in (False, True)]
        unbounded_occ = [r.rays(o, d, any_hit=True, reorder=ro, t_max=np.full(len(o), np.inf))["occluded"] for ro in (False, True)]
        r.close()
        check(f"{which} {mname}", got[0], p["exp"], inside, base, c["flat"], hier=mname == "hier")
        same(got[0], got[1])
        for ro in (0, 1):
            assert np.array_equal(occ[ro], got[0]["occluded"]), f"{which} {mname}: any_hit (reorder={ro}) != the nearest-hit pass's occluded"
            same(unbounded[ro], base)
            assert np.array_equal(unbounded_occ[ro], base_occ[ro]) and np.array_equal(base_occ[ro], base["occluded"])


# ---- 2. partial and idle wavefronts
@pytest.mark.parametrize("which,mname", [("big-scene", "hier"), ("macho-cows", "flat"), ("robot-alarm-clock", "kd"), ("robot-alarm-clock", "flat")])
def test_cut_batches_and_wavefronts_with_one_bounded_lane(oracle, host, H, which, mname):
    c = case(oracle, host, H, which)
    p = c["per"][mname]
    tr = {m[0]: m[1] for m in modes(H, oracle)}[mname]
    r = host.Renderer(c["sc"], tr, kd_depth=c["kd"])
    base = r.rays(c["o"], c["d"])
    full = filter_pass(base, p["inside"])
    for n in (1, 63, 64, 65, 130):
        for ro in (False, True):
            got = r.rays(c["o"][:n].copy(), c["d"][:n].copy(), reorder=ro, t_max=p["t_max"][:n].copy())
            same(got, {k: full[k][:n] for k in ALL})
            assert np.array_equal(bits(got["t"]), bits(p["exp"]["t"][:n])), (n, ro)
            occ = r.rays(c["o"][:n].copy(), c["d"][:n].copy(), any_hit=True, reorder=ro, t_max=p["t_max"][:n].copy())["occluded"]
            assert np.array_equal(occ, p["inside"][:n].astype(np.uint8)), (n, ro)
    # one lane with a valid bound among 63 empty ranges, in each of three wavefronts; a fourth wavefront with none
    live = np.flatnonzero(p["inside"])[:3]
    assert len(live) == 3
    idx = np.resize(np.flatnonzero(p["ref"]["id"] >= 0), 256)  # rays that WOULD hit, were their range not empty
    t_max = np.resize(EMPTY, 256)
    at = np.array([17, 64 + 63, 128])
    idx[at], t_max[at] = live, p["t_max"][live]
    inside = np.zeros(256, dtype=bool)
    inside[at] = True
    want = filter_pass({k: base[k][idx] for k in ALL}, inside)
    for ro in (False, True):
        got = r.rays(np.ascontiguousarray(c["o"][idx]), np.ascontiguousarray(c["d"][idx]), reorder=ro, t_max=t_max)
        same(got, want)
        assert np.array_equal(bits(got["t"][at]), bits(p["ref"]["t"][live])) and np.all(got["node"][at] >= 0)
        occ = r.rays(np.ascontiguousarray(c["o"][idx]), np.ascontiguousarray(c["d"][idx]), any_hit=True, reorder=ro, t_max=t_max)["occluded"]
        assert np.array_equal(occ, inside.astype(np.uint8))
    r.close()


# ---- 3. BoundingBox::test_hit with a bounded range
def test_a_ray_from_inside_a_cows_box_bounded_before_the_far_face(oracle, host, H):
    """Rays from the centre of each cow's box: the box's far face lies beyond t_max, a triangle before it (bounding_box.rs:104-116 must accept the mesh), and
    with t_max in front of the triangle the same rays miss."""
    c = case(oracle, host, H, "macho-cows")
    flat, a = c["flat"], c["ps"].arrays
    cows = np.flatnonzero(np.isin(flat["prim_type"], (2, 3)))
    assert len(cows) >= 2
    rng = np.random.default_rng(41)
    o, d, t_far = [], [], []
    voff = np.asarray(a["mesh_vert_off"], dtype=np.int64)
    for node in cows:
        m = int(flat["prim_data"][node])
        v = np.asarray(a["mesh_positions"]).reshape(-1, 3)[voff[m]:voff[m + 1]]
        lo, hi = v.min(axis=0), v.max(axis=0)
        centre = flat["trans"][node] @ np.append((lo + hi) / 2, 1.0)
        dirs = rng.normal(size=(400, 3))
        inv = flat["invtrans"][node]
        lo_d = dirs @ inv[:3, :3].T  # the directions in the mesh's space, where the ray starts at the box's centre: it leaves the box at ...
        with np.errstate(divide="ignore"):
            t_far.append(np.min((hi - lo) / 2 / np.abs(lo_d), axis=1))
        o.append(np.tile(centre[:3], (400, 1)))
        d.append(dirs)
    o, d, t_far = np.ascontiguousarray(np.concatenate(o)), np.ascontiguousarray(np.concatenate(d)), np.concatenate(t_far)
    for mname, tr, om in modes(H, oracle):
        ref = oracle_rays(oracle, c["ps"], o, d, om, c["kd"])
        own = np.isin(ref["id"], cows) & (ref["t"] < t_far * (1 - 1e-9))  # a triangle of the cow the ray starts in, in front of the far face
        assert own.sum() > 100, "rays from inside a cow must meet its triangles"
        t_max = np.where(own, (ref["t"] + t_far) / 2, np.inf)
        assert np.all((t_max > ref["t"])[own]) and np.all((t_max < t_far)[own])
        r = host.Renderer(c["sc"], tr, kd_depth=c["kd"])
        base = r.rays(o, d)
        for ro in (False, True):
            exp, inside = filtered(ref, t_max)
            assert inside[own].all()
            check(f"macho-cows {mname} from inside the box", r.rays(o, d, reorder=ro, t_max=t_max), exp, inside, base, flat, hier=mname == "hier")
            assert r.rays(o, d, any_hit=True, reorder=ro, t_max=t_max)["occluded"][own].all()
            short = np.where(own, ref["t"] / 2, np.inf)
            exp, inside = filtered(ref, short)
            assert not inside[own].any()
            check(f"macho-cows {mname} bounded in front of the triangle", r.rays(o, d, reorder=ro, t_max=short), exp, inside, base, flat, hier=mname == "hier")
            assert not r.rays(o, d, any_hit=True, reorder=ro, t_max=short)["occluded"][own].any()
        r.close()


# ---- 4. visibility between points
@pytest.mark.parametrize("which", ["big-scene", "macho-cows"])
def test_visibility_between_surface_points(oracle, host, H, which):
    """Segments between pairs of surface points of a primary-visibility pass: direction = b - a, t_max = 1. Unbounded, nearly every such ray is occluded by
    whatever lies behind b; bounded, the pairs that see each other are not."""
    c = case(oracle, host, H, which)
    sc = c["sc"]
    for mname, tr, om in modes(H, oracle):
        r = host.Renderer(sc, tr, kd_depth=c["kd"])
        prim = r.aov(sc.camera, 160, 96, want=("position", "node"))
        pts = prim["position"][prim["node"] >= 0]
        assert len(pts) > 2000
        rng = np.random.default_rng(3)
        a, b = pts[rng.integers(0, len(pts), size=6000)], pts[rng.integers(0, len(pts), size=6000)]
        keep = np.any(a != b, axis=1)
        o, d = np.ascontiguousarray(a[keep]), np.ascontiguousarray((b - a)[keep])
        ref = oracle_rays(oracle, c["ps"], o, d, om, c["kd"])
        exp, inside = filtered(ref, np.ones(len(o)))
        print(f"{which} {mname}: {len(o)} pairs, {int(inside.sum())} blocked, {int((ref['id'] >= 0).sum())} occluded without the bound")
        assert 0.01 * len(o) < inside.sum() < 0.99 * len(o) and (ref["id"] >= 0).sum() > inside.sum()  # both answers occur (b's own surface, met at t within rounding of 1, blocks about half the pairs that see each other)
        base = r.rays(o, d)
        for ro in (False, True):
            check(f"{which} {mname} point pairs", r.rays(o, d, reorder=ro, t_max=1.0), exp, inside, base, c["flat"], hier=mname == "hier")
            assert np.array_equal(r.rays(o, d, any_hit=True, reorder=ro, t_max=1.0)["occluded"], inside.astype(np.uint8))
        r.close()


# ---- 5. the pass among the others
def test_a_render_and_an_aov_pass_in_flight_around_a_segments_pass(oracle, host, H):
    """pt_render_device on both slots and a pt_aov_device pass in flight, then pt_segments_device on a stream: while it is open pt_rays_device, pt_rays,
    pt_segments_device and pt_segments are refused; pt_rays_finish closes it. Every result equals what the same calls give one after the other."""
    import device_glue
    from example_scenes import EXAMPLES
    n = 5000
    w, h, samples = 160, 96, 2
    bg = default_background(w, h)
    scene, cam0, _ = EXAMPLES["macho-cows"]()
    ps = oracle.pack(scene)  # (the scene as this test uploads it, through the C ABI)
    o, d = thinned_batch(oracle, ps, flat_of(oracle, ps, packed_tri_off(ps.arrays)), seed=77, n=n)
    ref = oracle_rays(oracle, ps, o, d, oracle.MODE_FLAT, -1)
    t_max = bounds_for(np.random.default_rng(9), ref["t"], d, 50.0)
    exp, inside = filtered(ref, t_max)
    assert inside.sum() > n // 5 and ((ref["id"] >= 0) & ~inside).sum() > n // 5
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
        d_bg, d_o, d_d, d_tm = dev(bg), dev(o), dev(d), dev(t_max)
        d_img, d_img2, d_depth, d_t, d_id = dev(nbytes=w * h * 3), dev(nbytes=w * h * 3), dev(nbytes=w * h * 8), dev(nbytes=n * 8), dev(nbytes=n * 4)
        st = H.PtStats()
        ap = H.PtAovParams(w, h, H.PtRect(0, 0, w - 1, h - 1), (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp))
        sp, sb = H.PtRaysParams(n, 0, 1), H.PtRaysBuffers(t=C.cast(d_t, H._dp), node=C.cast(d_id, H._ip))
        host_occ = np.zeros(n, dtype=np.uint8)
        hp, hb = H.PtRaysParams(n, 1, 0), H.PtRaysBuffers(occluded=host_occ.ctypes.data_as(H._u8p))
        dp = lambda x: x.ctypes.data_as(H._dp)

        def render(k, img):
            rp = H.PtRenderParams(w, h, H.PtRect(0, 0, w - 1, h - 1), samples, 10 + k, H.SAMPLE_RNG, 1, 0, 1, 0)
            return lib.pt_render_device(cx, C.byref(camera), d_bg, C.byref(rp), 0, img, C.c_void_p(lib.pt_context_stream(cx, k)))
        segments = lambda: lib.pt_segments_device(cx, C.byref(sp), d_o, d_d, d_tm, C.byref(sb), C.c_void_p(lib.pt_context_stream(cx, 0)))
        host_pass = lambda: lib.pt_segments(cx, C.byref(hp), dp(o), dp(d), dp(t_max), C.byref(hb), None)
        if overlapped:
            assert render(0, d_img) == 0 and render(1, d_img2) == 0 and lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0, lib.pt_last_error(cx)
            assert segments() == 0, lib.pt_last_error(cx)
            assert lib.pt_rays_device(cx, C.byref(sp), d_o, d_d, C.byref(sb), None) == H.ERR_ARGUMENT  # a segments pass is open: no ray pass of either kind
            assert segments() == H.ERR_ARGUMENT and host_pass() == H.ERR_ARGUMENT
            assert lib.pt_rays(cx, C.byref(hp), dp(o), dp(d), C.byref(hb), None) == H.ERR_ARGUMENT
            assert not host_occ.any()
            assert lib.pt_rays_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert lib.pt_rays_finish(cx, None) == H.ERR_ARGUMENT  # nothing open any more
            assert host_pass() == 0, lib.pt_last_error(cx)
            assert lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
        else:
            for k, img in ((0, d_img), (1, d_img2)):
                assert render(k, img) == 0 and lib.pt_render_finish(cx, C.byref(st)) == 0, lib.pt_last_error(cx)
            assert lib.pt_aov_device(cx, C.byref(camera), C.byref(ap), C.byref(ab), None) == 0 and lib.pt_aov_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert segments() == 0 and lib.pt_rays_finish(cx, None) == 0, lib.pt_last_error(cx)
            assert host_pass() == 0, lib.pt_last_error(cx)
        out = {"occ": host_occ}
        for name, ptr, arr in (("img", d_img, np.zeros((h, w, 3), dtype=np.uint8)), ("img2", d_img2, np.zeros((h, w, 3), dtype=np.uint8)), ("depth", d_depth, np.zeros((h, w))),
                               ("t", d_t, np.zeros(n)), ("id", d_id, np.zeros(n, dtype=np.int32))):
            assert lib.pt_copy_from_device(cx, arr.ctypes.data_as(C.c_void_p), ptr, arr.nbytes) == 0
            out[name] = arr
        for ptr in (d_bg, d_o, d_d, d_tm, d_img, d_img2, d_depth, d_t, d_id):
            lib.pt_device_free(cx, ptr)
        ctx.close()
        results.append(out)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), k
    got = results[1]
    assert got["img"].any() and got["img2"].any() and np.isfinite(got["depth"]).any()
    assert np.array_equal(bits(got["t"]), bits(exp["t"])) and np.array_equal(got["id"], exp["id"]) and np.array_equal(got["occ"], inside.astype(np.uint8))


def test_argument_errors_with_a_context(host, H):
    lib = H.lib()
    sc = host.Scene.example("primitives", assets=ASSETS)
    r = host.Renderer(sc, H.TRAVERSE_FLAT)
    ctx = r.context
    n = 100
    o, d, tm = np.zeros((n, 3)), np.ones((n, 3)), np.ones(n)
    t, occ = np.full(n, 3.0), np.full(n, 3, dtype=np.uint8)
    dp = lambda a: a.ctypes.data_as(H._dp)
    tb, ob = H.PtRaysBuffers(t=dp(t)), H.PtRaysBuffers(occluded=occ.ctypes.data_as(H._u8p))
    good = H.PtRaysParams(n, 0, 0)
    for fn in (lib.pt_segments, lib.pt_segments_device):
        assert fn(ctx, None, dp(o), dp(d), dp(tm), C.byref(tb), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), None, dp(d), dp(tm), C.byref(tb), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), None, dp(tm), C.byref(tb), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), dp(d), None, C.byref(tb), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), dp(d), dp(tm), C.byref(H.PtRaysBuffers()), None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(good), dp(o), dp(d), dp(tm), None, None) == H.ERR_ARGUMENT
        assert fn(ctx, C.byref(H.PtRaysParams(H.RAYS_MAX + 1, 0, 0)), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.ERR_ARGUMENT
        for a, ro in ((2, 0), (-1, 0), (0, 2), (0, -1)):
            assert fn(ctx, C.byref(H.PtRaysParams(n, a, ro)), dp(o), dp(d), dp(tm), C.byref(ob), None) == H.ERR_ARGUMENT, (a, ro)
        assert fn(ctx, C.byref(H.PtRaysParams(n, 1, 0)), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.ERR_ARGUMENT  # any_hit with more than `occluded`
        assert fn(ctx, C.byref(H.PtRaysParams(0, 0, 0)), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.OK  # n = 0: no launch, nothing written, nothing in flight
    assert np.all(t == 3.0) and np.all(occ == 3)
    assert lib.pt_rays_finish(ctx, None) == H.ERR_ARGUMENT  # nothing in flight
    assert lib.pt_segments(ctx, C.byref(good), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.OK
    bare = H.Context()
    assert lib.pt_segments(bare.handle, C.byref(good), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.ERR_NO_SCENE
    assert lib.pt_segments_device(bare.handle, C.byref(good), dp(o), dp(d), dp(tm), C.byref(tb), None) == H.ERR_NO_SCENE
    bare.close()
    empty = r.rays(np.zeros((0, 3)), np.zeros((0, 3)), t_max=np.zeros(0))
    assert empty["t"].shape == (0,) and empty["position"].shape == (0, 3)
    empty = r.rays(np.zeros((0, 3)), np.zeros((0, 3)), t_max=2.0)
    assert empty["node"].shape == (0,)
    r.close()
