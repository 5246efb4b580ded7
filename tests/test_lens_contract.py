"""The film's lens contract without a GPU (portrayer_amd/csrc/pt_lens.h): the numpy restatement of its steps 1 to 6 (tests/lens_restate.py)
against the host replay pt_test_lens_rays_host, which compiles the functions the kernel compiles, in every bit; the pinhole at aperture 0; and the properties
the lens points are chosen for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lens_restate import CENTRE, ORTHO, RNG, STEREO, THIN, camera_dict, draw, lens_points, normalized, replay, restate, xform_point  # noqa: E402
from test_ao_contract import ROT, same_bits  # noqa: E402

W, HGT = 19, 11
SAMPLES = (0, 7, 63, 64, 65, 4095)
LENSES = [(THIN, 0.35, 7.5, 1.0), (THIN, 0.0, 7.5, 1.0), (ORTHO, 0.0, 1.0, 3.25), (STEREO, 0.0, 1.0, float(np.tan(np.radians(170.0) / 4.0)))]
# eye, view direction, up, fovy in radians: none of the view's axes is a world axis
CAM10 = np.array([3.0, 2.5, 9.0, -0.31, -0.22, -1.0, 0.4, 1.0, 0.05, np.radians(50.0)])


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def pc():
    from portrayer_amd import host
    return host.camera(CAM10, W, HGT)


def cases():
    """Every pixel of the film, the four corners among them, with every sample index of SAMPLES"""
    xy = np.array([(x, y) for y in range(HGT) for x in range(W)], dtype=np.uint32)
    s = np.array(SAMPLES, dtype=np.uint32)
    return np.repeat(xy, len(s), axis=0), np.tile(s, len(xy))


def test_the_camera_is_not_axis_aligned(pc):
    m = np.array(list(pc.view_to_world)).reshape(4, 4)
    assert np.all(np.abs(m[:3, :3]) > 1e-3), "every entry of the rotation takes part in the products"
    assert pc.width == W and pc.height == HGT


@pytest.mark.parametrize("lens", LENSES, ids=["thin", "thin0", "ortho", "stereo"])
@pytest.mark.parametrize("mode", [CENTRE, RNG])
def test_the_restatement_equals_the_host_replay_in_every_bit(H, pc, lens, mode):
    xy, s = cases()
    corners = {(0, 0), (W - 1, 0), (0, HGT - 1), (W - 1, HGT - 1)}
    assert corners <= {tuple(int(v) for v in p) for p in xy}
    for seed in (0, 0x9e3779b97f4a7c15):
        O, D = restate(camera_dict(pc), lens, W, seed, mode, xy, s)
        O2, D2 = replay(H, pc, lens, W, HGT, seed, mode, xy, s)
        assert same_bits(O, O2), (lens, mode, seed)
        assert same_bits(D, D2), (lens, mode, seed)
        assert np.abs(np.sqrt((D * D).sum(1)) - 1.0).max() < 1e-15


def test_the_seed_the_sample_and_the_films_width_reach_the_rays(H, pc):
    xy, s = cases()
    lens = LENSES[0]
    base = replay(H, pc, lens, W, HGT, 7, RNG, xy, s)
    for other in (replay(H, pc, lens, W, HGT, 8, RNG, xy, s), replay(H, pc, lens, W + 1, HGT, 7, RNG, xy, s), replay(H, pc, lens, W, HGT, 7, RNG, xy, s + np.uint32(1))):
        assert not same_bits(base[0], other[0]) and not same_bits(base[1], other[1])
    # CENTRE fixes the point on the image, not the point on the lens: the origins are those of the jittered samples
    centre = replay(H, pc, lens, W, HGT, 7, CENTRE, xy, s)
    assert same_bits(centre[0], base[0]) and not same_bits(centre[1], base[1])


def pinhole(cam, seed, mode, xy, s, width):
    """pt_camera_ray at the jittered position (camera.rs:48-84), stated here once more"""
    x, y = xy[:, 0], xy[:, 1]
    pixel = y.astype(np.uint64) * np.uint64(width) + x.astype(np.uint64)
    jx, jy = (draw(seed, pixel, s, 0), draw(seed, pixel, s, 1)) if mode == RNG else (0.5, 0.5)
    sy = (y + jy) / cam["height"]
    view_y = (1.0 - 2.0 * sy) * cam["fov_factor"]
    sx = (x + jx) / cam["width"]
    view_x = (2.0 * sx - 1.0) * cam["aspect_ratio"] * cam["fov_factor"]
    world = xform_point(cam["view_to_world"], view_x, view_y, -1.0)
    return np.broadcast_to(cam["eye"], world.shape).copy(), normalized(world - cam["eye"])


@pytest.mark.parametrize("mode", [CENTRE, RNG])
def test_a_thin_lens_without_an_aperture_is_the_pinhole_bit_for_bit(H, pc, mode):
    xy, s = cases()
    for eye in (None, (-0.0, 2.5, 9.0), (3.0, -0.0, -0.0)):
        cam = H.PtCamera.from_buffer_copy(pc)
        if eye is not None:
            for k in range(3):
                cam.eye[k] = eye[k]
        for focus in (7.5, 1e-300):  # the focus takes no part
            O, D = replay(H, cam, (THIN, 0.0, focus, 1.0), W, HGT, 11, mode, xy, s)
            O2, D2 = pinhole(camera_dict(cam), 11, mode, xy, s, W)
            assert same_bits(O, O2) and same_bits(D, D2), (eye, focus)
            if eye is not None:
                assert np.array_equal(np.signbit(O[0]), np.signbit(np.array(eye))), "the eye's -0.0 is the origin's"
    # a real aperture moves the origin, and the plane of focus is where the rays of one pixel position meet
    O, D = replay(H, pc, (THIN, 0.35, 7.5, 1.0), W, HGT, 11, CENTRE, xy, s)
    O0, D0 = replay(H, pc, (THIN, 0.0, 7.5, 1.0), W, HGT, 11, CENTRE, xy, s)
    m = np.array(list(pc.view_to_world)).reshape(4, 4)
    axis = -m[:3, 2]
    t, t0 = 7.5 / (D @ axis), 7.5 / (D0 @ axis)
    assert np.abs((O + D * t[:, None]) - (O0 + D0 * t0[:, None])).max() < 1e-12


def test_lens_points_lie_in_the_unit_disc_and_64_consecutive_samples_fill_8_x_8_strata():
    pixel = np.full(4096, 5 * W + 3, dtype=np.uint64)
    s = np.arange(4096, dtype=np.uint32)
    lx, ly = lens_points(3, pixel, s)
    r2 = lx * lx + ly * ly
    assert r2.max() < 1.0 and r2.min() > 0.0
    # the angle is measured from the round's own rotation (PT_AO_ROT[j], j from the round's draw): the strata turn with it
    j = (draw(3, pixel, np.uint32(0x80000000) | (s >> np.uint32(6)), 0) * 256.0).astype(np.uint32)
    turn = np.arctan2(ROT[j, 1], ROT[j, 0]) / (2.0 * np.pi)
    angle = (np.arctan2(ly, lx) / (2.0 * np.pi) - turn) % 1.0
    first = np.floor(r2[:64] * 8).astype(int) * 8 + np.floor(angle[:64] * 8).astype(int)
    for rnd in (1, 63):
        later = np.floor(r2[64 * rnd:64 * rnd + 64] * 8).astype(int) * 8 + np.floor(angle[64 * rnd:64 * rnd + 64] * 8).astype(int)
        assert sorted(later) == list(range(64)), rnd
    assert sorted(first) == list(range(64)), "each of 8 x 8 strata of (radius^2, angle) holds one of the first 64 lens points"
    # every later round of 64 is the same set turned by its own rotation: its radii are round 0's, its strata of radius^2 hold 8 each
    for rnd in (1, 2, 63):
        assert np.allclose(r2[64 * rnd:64 * rnd + 64], r2[:64], rtol=0, atol=1e-15)
    rot = {(float(lx[64 * rnd]), float(ly[64 * rnd])) for rnd in range(64)}
    assert len(rot) > 48, "the rounds' rotations are draws of their own"
    # every power-of-two prefix of a round is stratified in radius^2
    for n in (2, 4, 8, 16, 32, 64):
        assert sorted(np.floor(r2[:n] * n).astype(int)) == list(range(n)), n


def test_the_hook_refuses_what_the_add_refuses(H, pc):
    xy, s = np.array([[0, 0]], dtype=np.uint32), np.array([0], dtype=np.uint32)
    nan, inf = float("nan"), float("inf")
    bad = [(3, 0.0, 1.0, 1.0), (-1, 0.0, 1.0, 1.0), (THIN, -1e-9, 1.0, 1.0), (THIN, nan, 1.0, 1.0), (THIN, inf, 1.0, 1.0), (THIN, 0.1, 0.0, 1.0), (THIN, 0.1, -1.0, 1.0),
           (THIN, 0.1, nan, 1.0), (THIN, 0.1, inf, 1.0), (ORTHO, 0.0, 1.0, 0.0), (ORTHO, 0.0, 1.0, nan), (STEREO, 0.0, 1.0, -2.0), (STEREO, 0.0, 1.0, inf)]
    for lens in bad:
        O, D = replay(H, pc, lens, W, HGT, 0, CENTRE, xy, s, expect=H.ERR_ARGUMENT)
        assert np.all(O == 7.0) and np.all(D == 7.0), lens
    # fields another model reads take no part
    replay(H, pc, (THIN, 0.1, 1.0, nan), W, HGT, 0, CENTRE, xy, s)
    replay(H, pc, (ORTHO, nan, -1.0, 2.0), W, HGT, 0, CENTRE, xy, s)
    replay(H, pc, LENSES[0], W, HGT, 0, 2, xy, s, expect=H.ERR_ARGUMENT)
    for off in ([[W, 0]], [[0, HGT]]):
        replay(H, pc, LENSES[0], W, HGT, 0, CENTRE, np.array(off, dtype=np.uint32), s, expect=H.ERR_ARGUMENT)
    assert H.lib().pt_test_lens_rays_host(None, None, W, HGT, 0, 0, 0, None, None, None, None) == H.ERR_ARGUMENT
