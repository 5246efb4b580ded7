"""A numpy restatement of the film's lens contract (portrayer_amd/csrc/pt_lens.h): steps 1 to 6 - which primary ray sample s of pixel (x, y)
casts through a thin lens, an orthographic or a stereographic camera. numpy's elementwise operations are separate correctly rounded f64 operations, nothing is
contracted, so this text and the functions the kernel compiles must agree in every bit (tests/test_lens_contract.py compares it with the host replay
pt_test_lens_rays_host); the GPU tests shade these rays with Renderer.radiance and fold them with pt_test_film_fold_host."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_ao_contract import DIRS, ROT, mix64  # noqa: E402  (PT_AO_DIRS and PT_AO_ROT are reused as they are)

THIN, ORTHO, STEREO = 0, 1, 2
CENTRE, RNG = 0, 1


def draw(seed, pixel, sample, k):
    """pt_rng_f64 (csrc/pt_math.h) over arrays of stream indices and sample indices; uint64 arithmetic wraps"""
    with np.errstate(over="ignore"):
        key0 = mix64(np.array([seed], dtype=np.uint64) + np.uint64(0x9e3779b97f4a7c15))
        key = mix64(key0 ^ (pixel.astype(np.uint64) * np.uint64(0xd1342543de82ef95) + np.uint64(0x632be59bd9b4e019)))
        r = mix64(key ^ ((sample.astype(np.uint64) << np.uint64(32)) | np.uint64(k)))
    return (r >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def camera_dict(pc):
    """A pt_camera (portrayer_amd._hip.PtCamera) as the dict restate() reads"""
    return dict(eye=np.array(list(pc.eye)), view_to_world=np.array(list(pc.view_to_world)), fov_factor=pc.fov_factor, aspect_ratio=pc.aspect_ratio, width=pc.width,
                height=pc.height)


def replay(H, pc, lens, width, height, seed, sample_mode, xy, s, expect=0):
    """pt_test_lens_rays_host: the contract by the functions the kernel compiles. lens: (model, aperture, focus, extent). -> origins, directions (n, 3)"""
    import ctypes as C
    xy, s = np.ascontiguousarray(xy, dtype=np.uint32), np.ascontiguousarray(s, dtype=np.uint32)
    n = len(s)
    O, D = np.full((n, 3), 7.0), np.full((n, 3), 7.0)
    u32p = C.POINTER(C.c_uint32)
    rc = H.lib().pt_test_lens_rays_host(C.byref(pc), C.byref(H.PtLens(*lens)), width, height, seed, sample_mode, n, xy.ctypes.data_as(u32p), s.ctypes.data_as(u32p),
                                        O.ctypes.data_as(H._dp), D.ctypes.data_as(H._dp))
    assert rc == expect, rc
    return O, D


def xform_point(m, x, y, z):
    """pt_xform_point: rows 0 .. 2 of the row-major 4x4 `m` (16 doubles), w = 1, summed left to right"""
    return np.stack([((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)], axis=-1)


def normalized(v):
    return v / np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])[..., None]


def lens_points(seed, pixel, s):
    """Step 3: (lx, ly) of samples `s` of the pixels with stream indices `pixel`"""
    k, r = s & np.uint32(63), s >> np.uint32(6)
    j = (draw(seed, pixel, np.uint32(0x80000000) | r, 0) * 256.0).astype(np.uint32)
    c, sn = ROT[j, 0], ROT[j, 1]
    px, py = DIRS[k, 0], DIRS[k, 1]
    return c * px - sn * py, sn * px + c * py


def restate(cam, lens, width, seed, sample_mode, xy, s):
    """Steps 1 to 6 in numpy. cam: a pt_camera's fields as a dict (eye (3,), view_to_world (16,), fov_factor, aspect_ratio, width, height); lens: (model,
    aperture, focus, extent); xy (n, 2) and s (n,) uint32. -> origins (n, 3), directions (n, 3)."""
    model, aperture, focus, extent = lens
    xy, s = np.asarray(xy, dtype=np.uint32), np.asarray(s, dtype=np.uint32)
    x, y = xy[:, 0], xy[:, 1]
    pixel = y.astype(np.uint64) * np.uint64(width) + x.astype(np.uint64)
    eye, m = np.asarray(cam["eye"], dtype=np.float64), np.asarray(cam["view_to_world"], dtype=np.float64)
    with np.errstate(all="ignore"):
        if sample_mode == RNG:
            jx, jy = draw(seed, pixel, s, 0), draw(seed, pixel, s, 1)
        else:
            jx = jy = np.full(len(s), 0.5)
        sx, sy = x.astype(np.float64) + jx, y.astype(np.float64) + jy
        ndc_x, ndc_y = sx / cam["width"], sy / cam["height"]
        if model == THIN:
            view_y = (1.0 - 2.0 * ndc_y) * cam["fov_factor"]
            view_x = ((2.0 * ndc_x - 1.0) * cam["aspect_ratio"]) * cam["fov_factor"]
            world = xform_point(m, view_x, view_y, -1.0)
            D = world - eye
            if aperture == 0.0:
                return np.broadcast_to(eye, D.shape).copy(), normalized(D)
            lx, ly = lens_points(seed, pixel, s)
            R, U = m[[0, 4, 8]], m[[1, 5, 9]]
            e = (R[None, :] * lx[:, None] + U[None, :] * ly[:, None]) * aperture
            return eye + e, normalized(D - e / focus)
        u = ((2.0 * ndc_x - 1.0) * cam["aspect_ratio"]) * extent
        v = (1.0 - 2.0 * ndc_y) * extent
        if model == ORTHO:
            o = xform_point(m, u, v, 0.0)
            return o, normalized(xform_point(m, u, v, -1.0) - o)
        q = u * u + v * v
        world = xform_point(m, 2.0 * u, 2.0 * v, q - 1.0)
        return np.broadcast_to(eye, world.shape).copy(), normalized(world - eye)
