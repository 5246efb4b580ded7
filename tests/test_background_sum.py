"""pt_background_sum (pt_shade.h), the sum the finish kernel gives a pixel that the render kernel was never dealt (pt_pixel_list.h: the queue): every sample
of such a pixel is the background colour, and the sum must be the one the render kernel's chunk loop and the finish kernel's pass over the chunk sums would have formed -
the summation contract, add for add:

  a chunk's first sample is assigned, the rest of its min(8, samples - 8 k) samples are added left to right; the pixel's first chunk is assigned, the other chunks are
  added in ascending order.

The host build of the function (pt_test_background_sum, no GPU) against that fold written out in numpy f64 scalars. Bit patterns are compared, not values: -0.0 stays
-0.0, an infinity and a NaN come out as the adds leave them, and 1e-300 and 1e300 neither flush nor take a short cut through a product."""
import ctypes as C

import numpy as np
import pytest

SAMPLES = [57, 60, 63, 64, 113, 121, 128]
COLOURS = [0.1, 1.0 / 3.0, 1e-300, 1e300, -0.0, float("inf"), float("nan")]


def contract_fold(colour: float, samples: int) -> np.float64:
    """The contract, one f64 add at a time."""
    c = np.float64(colour)
    total = None
    with np.errstate(all="ignore"):
        for first in range(0, samples, 8):
            n = min(8, samples - first)
            chunk = c  # the chunk's first sample: assigned
            for _ in range(1, n):
                chunk = np.float64(chunk + c)
            total = chunk if total is None else np.float64(total + chunk)  # the first chunk: assigned
    return total


def bits(v) -> np.ndarray:
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def lib():
    from portrayer_amd import _hip
    return _hip.lib()


def device_form(lib, rgb, samples):
    dp = C.POINTER(C.c_double)
    src = np.ascontiguousarray(rgb, dtype=np.float64)
    out = np.full(3, 123.0)
    assert lib.pt_test_background_sum(src.ctypes.data_as(dp), samples, out.ctypes.data_as(dp)) == 0
    return out


@pytest.mark.parametrize("samples", SAMPLES)
def test_every_colour_alone(lib, samples):
    for colour in COLOURS:
        got = device_form(lib, [colour, colour, colour], samples)
        want = contract_fold(colour, samples)
        assert np.array_equal(bits(got), bits([want] * 3)), (samples, colour, got, want)


@pytest.mark.parametrize("samples", SAMPLES)
def test_the_channels_do_not_mix(lib, samples):
    """Three different colours in one pixel, every rotation of the list: each channel is its own fold."""
    for k in range(len(COLOURS)):
        rgb = [COLOURS[k], COLOURS[(k + 1) % len(COLOURS)], COLOURS[(k + 3) % len(COLOURS)]]
        got = device_form(lib, rgb, samples)
        want = [contract_fold(c, samples) for c in rgb]
        assert np.array_equal(bits(got), bits(want)), (samples, rgb, got, want)


def test_the_fold_is_no_product():
    """What the test compares with really is a fold: for 0.1 and 64 samples it differs from 64 * 0.1, and -0.0 keeps its sign."""
    assert bits(contract_fold(0.1, 57))[0] != bits(np.float64(57) * np.float64(0.1))[0] or bits(contract_fold(1.0 / 3.0, 121))[0] != bits(np.float64(121) / 3.0)[0]
    assert np.signbit(contract_fold(-0.0, 64))


def test_arguments_are_checked(lib):
    out = np.zeros(3)
    dp = C.POINTER(C.c_double)
    assert lib.pt_test_background_sum(None, 64, out.ctypes.data_as(dp)) != 0
    assert lib.pt_test_background_sum(out.ctypes.data_as(dp), 0, out.ctypes.data_as(dp)) != 0
