"""What the device passes beside the render share (pt_context.h: PtPass; pt_api.hip: the pt_pass_* functions), pinned where the per-pass tests leave it open: the exact
words of every "in flight" refusal and of every _finish with nothing open, each pass's flag apart from the others', a call with nothing to do (n = 0, an
inverted slice) that queues nothing and reports 0 ms, the film's passes kept as the radiance pass's, and a context destroyed while all three passes are open.
The `primitives` scene, a 16x16 image, 64 rays: the words and the bookkeeping do not depend on the size."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from scene_dsl import ASSETS  # noqa: E402

pytestmark = pytest.mark.gpu

W = 16
N = 64


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def host():
    from portrayer_amd import host
    return host


class Calls:
    """One renderer on the scene, every array of the passes in device memory, and the passes' _device / host / _finish calls with their arguments bound."""

    def __init__(self, host, H):
        self.H, self.lib = H, H.lib()
        self.sc = host.Scene.example("primitives", assets=ASSETS)
        self.r = host.Renderer(self.sc, H.TRAVERSE_FLAT)
        self.ctx = ctx = self.r.context
        lib = self.lib
        self.cam = host.camera(self.sc.camera, W, W)
        rng = np.random.default_rng(3)
        self.o, self.d = rng.uniform(-4, 4, size=(N, 3)), rng.normal(size=(N, 3))
        self.t_max = np.full(N, 50.0)
        self.bg = rng.uniform(size=(W, W, 3))
        self.held = []

        def dev(nbytes, src=None):
            p = C.c_void_p()
            assert lib.pt_device_alloc(ctx, nbytes, C.byref(p)) == H.OK
            if src is not None:
                assert lib.pt_copy_to_device(ctx, p, src.ctypes.data_as(C.c_void_p), src.nbytes) == H.OK
            self.held.append(p)
            return p
        d_o, d_d, d_tm, d_bg = dev(N * 24, self.o), dev(N * 24, self.d), dev(N * 8, self.t_max), dev(self.bg.nbytes, self.bg)
        d_depth, d_t, d_rgb = dev(W * W * 8), dev(N * 8), dev(N * 24)
        full = H.PtRect(0, 0, W - 1, W - 1)
        ap = H.PtAovParams(W, W, full, (C.c_double * 2)(0.5, 0.5))
        ab = H.PtAovBuffers(depth=C.cast(d_depth, H._dp))
        self.h_depth, self.h_t, self.h_rgb = np.zeros((W, W)), np.zeros(N), np.zeros((N, 3))
        hab = H.PtAovBuffers(depth=self.h_depth.ctypes.data_as(H._dp))
        rb = H.PtRaysBuffers(t=C.cast(d_t, H._dp))
        hrb = H.PtRaysBuffers(t=self.h_t.ctypes.data_as(H._dp))
        dp = lambda a: a.ctypes.data_as(H._dp)
        cam = self.cam
        self.ms = C.c_double(-1.0)
        ms = C.byref(self.ms)
        self.aov_device = lambda: lib.pt_aov_device(ctx, C.byref(cam), C.byref(ap), C.byref(ab), None)
        self.aov = lambda: lib.pt_aov(ctx, C.byref(cam), C.byref(ap), C.byref(hab), ms)
        self.rays_device = lambda n=N: lib.pt_rays_device(ctx, C.byref(H.PtRaysParams(n, 0, 0)), d_o, d_d, C.byref(rb), None)
        self.segments_device = lambda n=N: lib.pt_segments_device(ctx, C.byref(H.PtRaysParams(n, 0, 1)), d_o, d_d, d_tm, C.byref(rb), None)
        self.rays = lambda n=N: lib.pt_rays(ctx, C.byref(H.PtRaysParams(n, 0, 0)), dp(self.o), dp(self.d), C.byref(hrb), ms)
        self.segments = lambda n=N: lib.pt_segments(ctx, C.byref(H.PtRaysParams(n, 0, 0)), dp(self.o), dp(self.d), dp(self.t_max), C.byref(hrb), ms)
        self.radiance_device = lambda n=N: lib.pt_radiance_device(ctx, C.byref(H.PtRadianceParams(n, 1, 0, 0, 0, 0)), d_o, d_d, d_bg, d_rgb, None)
        self.radiance = lambda n=N: lib.pt_radiance(ctx, C.byref(H.PtRadianceParams(n, 0, 0, 0, 0, 0)), dp(self.o), dp(self.d), dp(self.bg), dp(self.h_rgb), ms)
        self.films = []
        for _ in (0, 1):
            f = C.c_void_p()
            assert lib.pt_film_create_moments(ctx, W, W, C.byref(f)) == H.OK
            self.films.append(f)
        inverted = H.PtRect(5, 0, 4, W - 1)
        fp = lambda slice_, samples: C.byref(H.PtFilmParams(slice_, samples, 2, H.SAMPLE_RNG, 0))
        self.film_add_device = lambda k=0, samples=3, slice_=full: lib.pt_film_add_device(ctx, self.films[k], C.byref(cam), d_bg, fp(slice_, samples), None)
        self.film_add = lambda k=0, samples=3, slice_=full: lib.pt_film_add(ctx, self.films[k], C.byref(cam), dp(self.bg), fp(slice_, samples), ms)
        self.inverted = inverted
        d_budget = dev(W * W * 4, np.full((W, W), 2, dtype=np.uint32))
        mp = C.byref(H.PtFilmMapParams(full, 9, 2, H.SAMPLE_RNG, 0))
        self.film_add_map_device = lambda k=0: lib.pt_film_add_map_device(ctx, self.films[k], C.byref(cam), d_bg, mp, d_budget, None)
        self.counts = np.zeros((W, W), dtype=np.uint32)
        self.film_counts = lambda k=0: lib.pt_film_counts(ctx, self.films[k], self.counts.ctypes.data_as(H._up))
        self.finish = {"aov": lambda: lib.pt_aov_finish(ctx, ms), "rays": lambda: lib.pt_rays_finish(ctx, ms), "radiance": lambda: lib.pt_radiance_finish(ctx, ms)}

    def says(self, rc, words):
        assert rc == self.H.ERR_ARGUMENT and self.lib.pt_last_error(self.ctx) == words, (rc, self.lib.pt_last_error(self.ctx))

    def ok(self, rc):
        assert rc == self.H.OK, (rc, self.lib.pt_last_error(self.ctx))

    def close(self):
        for p in self.held:
            self.lib.pt_device_free(self.ctx, p)
        self.r.close()


NONE_OPEN = {"aov": b"no pt_aov_device pass in flight", "rays": b"no pt_rays_device / pt_segments_device pass in flight", "radiance": b"no pt_radiance_device pass in flight"}
OPEN = {"aov": b"a pt_aov_device pass is in flight: pt_aov_finish first", "rays": b"a pt_rays_device / pt_segments_device pass is in flight: pt_rays_finish first",
        "radiance": b"a pt_radiance_device pass is in flight: pt_radiance_finish first"}
FILM_OPEN = b"a pt_radiance_device / pt_film_add_device pass is in flight: pt_radiance_finish first"


def test_every_pass_keeps_its_own_flag_and_its_own_words(host, H):
    k = Calls(host, H)
    queue = {"aov": (k.aov_device, k.aov), "rays": (k.rays_device, k.rays, k.segments_device, k.segments), "radiance": (k.radiance_device, k.radiance)}
    for name in ("aov", "rays", "radiance"):
        k.says(k.finish[name](), NONE_OPEN[name])
    for name, calls in queue.items():
        for opener in calls[0::2]:  # the _device forms; every form of the pass is refused while one is open, no other pass is
            k.ok(opener())
            for call in calls:
                k.says(call(), OPEN[name])
            for other in queue:
                if other != name:
                    k.says(k.finish[other](), NONE_OPEN[other])
                    k.ok(queue[other][1]())  # the other passes' host forms run beside it
            k.ms.value = -1.0
            k.ok(k.finish[name]())
            assert k.ms.value > 0.0
            k.says(k.finish[name](), NONE_OPEN[name])
    # all three open at once, closed in another order
    k.ok(k.aov_device()), k.ok(k.segments_device()), k.ok(k.radiance_device())
    k.ok(k.finish["rays"]()), k.ok(k.finish["radiance"]()), k.ok(k.finish["aov"]())
    k.close()


def test_a_call_with_nothing_to_do_queues_nothing_and_reports_zero(host, H):
    k = Calls(host, H)
    for call in (k.rays, k.segments, k.radiance):
        k.ms.value = -1.0
        k.ok(call(0))
        assert k.ms.value == 0.0
    k.ms.value = -1.0
    k.ok(k.film_add(0, 3, k.inverted))
    assert k.ms.value == 0.0
    k.ok(k.rays_device(0)), k.ok(k.segments_device(0)), k.ok(k.radiance_device(0)), k.ok(k.film_add_device(0, 3, k.inverted))
    for name in ("rays", "radiance"):
        k.says(k.finish[name](), NONE_OPEN[name])
    k.ok(k.film_counts())
    assert not k.counts.any()
    k.close()


def test_a_films_pass_is_the_radiance_passes(host, H):
    k = Calls(host, H)
    lib, ctx = k.lib, k.ctx
    for opener in (k.film_add_device, k.film_add_map_device):
        k.ok(opener(0))
        k.says(k.radiance_device(), OPEN["radiance"])
        k.says(k.radiance(), OPEN["radiance"])
        for refused in (k.film_add_device, k.film_add, k.film_add_map_device):
            for film in (0, 1):
                k.says(refused(film), FILM_OPEN)
        who = b"pt_film_counts: a pt_film_add_device pass of this film is in flight: pt_radiance_finish first"
        k.says(k.film_counts(0), who)  # only the open film is busy
        k.ok(k.film_counts(1))
        k.says(k.finish["aov"](), NONE_OPEN["aov"]), k.says(k.finish["rays"](), NONE_OPEN["rays"])
        k.ms.value = -1.0
        k.ok(k.finish["radiance"]())
        assert k.ms.value > 0.0
        k.says(k.finish["radiance"](), NONE_OPEN["radiance"])
        k.ok(k.film_counts(0))
    assert np.all(k.counts == 3 + 2)  # the add's three samples, then the map's two
    # a radiance pass open: the films' adds are refused, their state may be read
    k.ok(k.radiance_device())
    k.says(k.film_add_device(0), FILM_OPEN)
    k.ok(k.film_counts(0))
    k.ok(k.finish["radiance"]())
    assert lib.pt_film_destroy(ctx, k.films[0]) == H.OK
    k.close()  # (the second film dies with the context)


def test_a_context_destroyed_with_every_pass_open_waits_for_them(host, H):
    k = Calls(host, H)
    k.ok(k.aov_device()), k.ok(k.rays_device()), k.ok(k.radiance_device())
    k.r.close()  # pt_context_destroy: waits for the three passes, then frees what they read
    k2 = Calls(host, H)
    k2.ok(k2.film_add_device(0))
    k2.r.close()
    k3 = Calls(host, H)  # the device is as usable as before
    k3.ok(k3.aov()), k3.ok(k3.rays()), k3.ok(k3.radiance())
    assert k3.h_depth.any() and k3.h_t.any() and k3.h_rgb.any()
    k3.close()
