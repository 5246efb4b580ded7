"""GPU parity of the device library alone (C ABI of include/portrayer_hip.h), inputs flattened by the
oracle so that only the HIP kernels are under test. Bar: ray parameter / node index bit-exact;
f64 colours bit-exact (the device pow is glibc's, pt_pow.h), u8 pixels identical."""
import numpy as np
import pytest

from example_scenes import EXAMPLES, big_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from portrayer_amd import _hip as H
    c = H.Context(0)
    yield c
    c.close()


from ulp import assert_ulp, ulp_diff  # noqa: E402


def test_device_arithmetic_is_ieee(ctx):
    """sqrt and / must be correctly rounded and a*b+c must not be fused (SURVEY App.B.5, H2)."""
    rng = np.random.default_rng(1)
    a = np.exp(rng.uniform(-40, 40, 200000)) * rng.choice([1.0, 1.0, 1.0], 200000)
    b = np.exp(rng.uniform(-40, 40, 200000)) * rng.choice([-1.0, 1.0], 200000)
    assert np.array_equal(ctx.math(0, a, b), np.sqrt(a))
    assert np.array_equal(ctx.math(1, a, b), a / b)
    x = rng.uniform(-2, 2, 200000); y = rng.uniform(-2, 2, 200000)
    assert np.array_equal(ctx.math(3, x, y), x * y + x)


def test_short_division_of_the_kd_walk_is_the_hardware_division(ctx):
    """Every straddled split of the k-d walk divides by the same direction component: pt_div_fast() finishes a division in three
    instructions from a reciprocal refined once per ray (pt_walk_kd.h). It must be `/` bit for bit wherever its exponent test admits the
    operands (biased exponents in [640, 1407]); everything else - zeros, denormals, infinities, NaNs, huge and tiny values - must be
    refused (NaN marker here; the walk then takes the real division). Random mantissas over the whole window, its edges, exact
    quotients, powers of two, operands one ulp apart."""
    rng = np.random.default_rng(9)
    n = 400000
    def rnd(lo, hi, k):
        return np.ldexp(rng.uniform(0.5, 1.0, k), rng.integers(lo, hi, k).astype(np.int32)) * rng.choice([-1.0, 1.0], k)
    a = np.concatenate([rnd(-382, 385, n), rnd(-40, 40, n), rnd(-382, -370, n // 4), rnd(373, 385, n // 4), rnd(-1070, 1024, n // 4)])
    b = np.concatenate([rnd(-382, 385, n), rnd(-40, 40, n), rnd(373, 385, n // 4), rnd(-382, -370, n // 4), rnd(-1070, 1024, n // 4)])
    ints = rng.integers(1, 1 << 20, n // 4).astype(np.float64)
    a = np.concatenate([a, ints * rng.integers(1, 1 << 20, n // 4), np.ldexp(1.0, rng.integers(-300, 300, 1000)), np.nextafter(b[:1000], np.inf),
                        np.array([0.0, -0.0, np.inf, np.nan, 5e-324, 1e-310, 1.0, 1.0, 1.0, 3.0])])
    b = np.concatenate([b, ints, np.ldexp(1.0, rng.integers(-300, 300, 1000)) * 3.0, b[:1000],
                        np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, np.inf, np.nan, 5e-324])])
    got = ctx.math(7, a, b)
    def biased(x):
        return ((x.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    admitted = (biased(a) >= 640) & (biased(a) <= 1407) & (biased(b) >= 640) & (biased(b) <= 1407)
    assert np.isnan(got[~admitted]).all(), "an operand outside the window was not refused"
    with np.errstate(all="ignore"):
        exact = a / b
    assert admitted.sum() > 2 * n
    assert np.array_equal(got[admitted].view(np.uint64), exact[admitted].view(np.uint64))
    assert np.array_equal(ctx.math(1, a[admitted], b[admitted]).view(np.uint64), exact[admitted].view(np.uint64))  # and the device's `/` is numpy's


def libm_pow(x, y):
    """x ** y by this machine's libm (what the oracle and the reference call), NOT numpy's own vectorised pow"""
    from portrayer_amd import _hip as H
    port = np.empty_like(x); libm = np.empty_like(x)
    assert H.lib().pt_test_pow_host(x.size, x.ctypes.data_as(H._dp), y.ctypes.data_as(H._dp), port.ctypes.data_as(H._dp), libm.ctypes.data_as(H._dp)) == 0
    return libm


def test_device_pow_is_glibc_pow_bit_for_bit(ctx):
    """pow (gamma render.rs:47, specular material.rs:200) is the only libm call on the path: the kernels' pt_pow (pt_pow.h, glibc's
    algorithm restated) against the host's libm on the exponents the renderer uses, 0 ulp."""
    rng = np.random.default_rng(2)
    n = 200000
    base = np.concatenate([rng.uniform(0.0, 1.5, n), rng.uniform(0.0, 1.0, n), np.array([0.0, 1.0, 0.5, 1e-300, 1e-320, 4.0, np.inf])])
    e = np.concatenate([np.where(rng.random(n) < 0.5, 1.0 / 2.2, rng.choice([4.0, 80.0, 100.0, 200.0, 4000.0], n)), 4.0 * rng.integers(1, 64, n).astype(np.float64),
                        np.array([100.0, 100.0, 1.0 / 2.2, 1.0 / 2.2, 0.5, 1.0 / 2.2, 1.0 / 2.2])])
    got, exp = ctx.math(2, base, e), libm_pow(base, e)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), f"max {ulp_diff(got, exp).max()} ulp"
    x = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-1070, 1024, n).astype(np.int32)); y = rng.uniform(-300.0, 300.0, n)  # the whole function, not only the renderer's corner of it
    got, exp = ctx.math(2, x, y), libm_pow(x, y)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), f"max {ulp_diff(got, exp).max()} ulp"
    d = ulp_diff(ctx.math(6, base[:n], e[:n]), libm_pow(base[:n], e[:n]))  # for the record: the device library's own pow
    print(f"ocml pow: {100.0 * (d == 0).mean():.3f} % bit-equal to glibc, max {d.max()} ulp")


def libm(op, a, b):
    """The host's libm (glibc) through the library's own entry point - not numpy, whose vectorised routines are not glibc's on every machine."""
    from portrayer_amd import _hip as H
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    out = np.empty_like(a)
    assert H.lib().pt_test_libm_host(op, a.size, a.ctypes.data_as(H._dp), b.ctypes.data_as(H._dp), out.ctypes.data_as(H._dp)) == 0
    return out


def test_device_atan2_acos_against_glibc(ctx):
    """The other libm calls on the device: sphere texture coordinates (sphere.rs:57-60, pt_apply_maps) go through atan2 and
    acos. Their results only select a texel, so a last-bit difference matters only on a texel boundary; the measured bound
    against glibc itself (pt_test_libm_host) is written here so that a device-library change shows. (glibc 2.35's atan2 - about 1,400
    instructions in this image's stripped libm - was not restated like pow, and it is not correctly rounded either - 0.1 % of its results are not the
    nearest double, profiles/tools/glibc_atan2_rounding.py -, so a correctly rounded device routine would not equal it.)"""
    rng = np.random.default_rng(5)
    n = 200000
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]  # points on the unit sphere, like hit points
    exp_a, exp_c = libm(4, -d[:, 2], d[:, 0]), libm(5, d[:, 1], d[:, 1])
    got_a, got_c = ctx.math(4, -d[:, 2], d[:, 0]), ctx.math(5, d[:, 1], d[:, 1])
    da, dc = ulp_diff(got_a, exp_a), ulp_diff(got_c, exp_c)
    print(f"atan2: {100.0 * (da == 0).mean():.3f} % bit-equal to glibc, max {da.max()} ulp; acos: {100.0 * (dc == 0).mean():.3f} %, max {dc.max()} ulp")
    assert_ulp(got_a, exp_a, 2, "atan2")
    assert_ulp(got_c, exp_c, 1, "acos")
    # for the record: numpy's own routines against glibc on this machine
    print(f"numpy arctan2 vs glibc: max {ulp_diff(np.arctan2(-d[:, 2], d[:, 0]), exp_a).max()} ulp; arccos: max {ulp_diff(np.arccos(d[:, 1]), exp_c).max()} ulp")


SMALL = {"single-triangle": (160, 120), "primitives-simple": (182, 102), "macho-cows": (96, 96),
         "entering-the-mirror-dimension": (160, 120), "big-scene": (198, 102)}


@pytest.mark.parametrize("name", list(SMALL))
@pytest.mark.parametrize("mode", ["flat", "kd"])
def test_render_matches_oracle(ctx, oracle, name, mode):
    import device_glue as G
    from portrayer_amd import _hip as H
    scene, cam, _ = EXAMPLES[name]()
    w, h = SMALL[name]
    ds = G.DeviceScene(scene, H.TRAVERSE_KD if mode == "kd" else H.TRAVERSE_FLAT, kd_depth=10)
    ds.upload(ctx)
    rgb, linear, st = G.render(ctx, cam, w, h, stats=True)
    ref = oracle.render(ds.ps, cam, w, h, mode=oracle.MODE_KD if mode == "kd" else oracle.MODE_FLAT)
    assert st["stack_overflow"] == 0 and st["kd_plane_miss"] == ref.stats["kd_plane_miss"]
    for k in ("primary", "shadow", "reflect", "refract", "hits"):
        assert st[k] == ref.stats[k], k
    assert st["depth11_skipped"] == ref.stats["depth11"]
    d = ulp_diff(linear, ref.linear)
    print(f"{name}/{mode}: linear bit-equal {100.0 * (d == 0).mean():.4f} %, max {d.max()} ulp; kernel {st['kernel_ms']:.2f} ms")
    assert np.array_equal(rgb, ref.rgb)
    assert_ulp(linear, ref.linear, 0, f"{name}/{mode}")  # bit-identical: the device pow is glibc's (pt_pow.h)
    if mode == "kd":  # same tree, same order; shadow rays stop at the first hit of a leaf, the oracle finishes the leaf
        assert st["n_analytic"] <= ref.stats["n_analytic"]
        if ref.stats["n_tri"] == 0:  # with meshes n_inner also counts the build's own triangle-tree nodes
            assert st["n_inner"] <= ref.stats["n_split"]


@pytest.mark.parametrize("mode", ["flat", "kd"])
def test_cast_rays_bit_exact(ctx, oracle, mode):
    import device_glue as G
    from portrayer_amd import _hip as H
    scene, cam, (w, h) = big_scene()
    ds = G.DeviceScene(scene, H.TRAVERSE_KD if mode == "kd" else H.TRAVERSE_FLAT)
    ds.upload(ctx)
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(0, w, 50000), rng.uniform(0, h, 50000)], axis=1)
    o, d = oracle.camera_rays(cam, w, h, xy)
    t, node, sub = ctx.cast_rays(o, d)
    rt, rid, _, _ = oracle.cast_rays(ds.ps, o, d, mode=oracle.MODE_KD if mode == "kd" else oracle.MODE_FLAT)
    assert np.array_equal(node, rid)
    assert np.array_equal(t, rt)
    # any-hit: same hit / miss decision
    t2, node2, _ = ctx.cast_rays(o, d, any_hit=True)
    assert np.array_equal(node2 >= 0, rid >= 0)


def test_multisample_rng_and_slice(ctx, oracle):
    import device_glue as G
    from portrayer_amd import _hip as H
    scene, cam, _ = EXAMPLES["entering-the-mirror-dimension"]()
    ds = G.DeviceScene(scene, H.TRAVERSE_FLAT)
    ds.upload(ctx)
    w, h = 120, 90
    into = np.full((h, w, 3), 7, dtype=np.uint8)
    rgb, linear, st = G.render(ctx, cam, w, h, samples=4, seed=42, sample_mode=H.SAMPLE_RNG, rect=(10, 5, 99, 70), into=into)
    ref_into = np.full((h, w, 3), 7, dtype=np.uint8)
    ref = oracle.render(ds.ps, cam, w, h, samples=4, seed=42, jitter=oracle.JITTER_RNG, mode=oracle.MODE_FLAT, rect=(10, 5, 99, 70), into=ref_into)
    assert np.array_equal(rgb, ref.rgb)
    assert (rgb[0, 0] == 7).all() and (rgb[71:, :] == 7).all(), "pixels outside the slice must be untouched (render.rs:135-138)"
    assert_ulp(linear[5:71, 10:100], ref.linear[5:71, 10:100], 0)
