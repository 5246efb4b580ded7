"""The plan of pt_film_add_map without a GPU: pt_test_film_plan_host builds, from the functions the plan kernels call (pt_film_map_slot_round,
pt_film_map_entry, pt_slot_to_pixel), the list the sampling kernel walks in launch round r - one entry (slot << 3) | j per sample, in ascending (slot, j) order,
slot = the pixel's place in the slice's 8x8 tiles (row-major over tiles, rows inside a tile). Against numpy's own enumeration."""
import ctypes as C

import numpy as np
import pytest

LW = 8  # PT_FILM_LW
BUDGETS = np.array([0, 1, 3, 8, 9, 17], dtype=np.uint32)


@pytest.fixture(scope="module")
def H():
    from portrayer_amd import _hip
    return _hip


def numpy_plan(w, h, rect, budget, max_samples, rnd):
    """The list of round `rnd`, and the (slot -> pixel) table it was made from."""
    x0, y0, x1, y1 = rect
    tiles_x, tiles_y = (x1 - x0 + 8) // 8, (y1 - y0 + 8) // 8
    out = []
    for slot in range(tiles_x * tiles_y * 64):
        tile, j = slot >> 6, slot & 63
        x, y = x0 + (tile % tiles_x) * 8 + (j & 7), y0 + (tile // tiles_x) * 8 + (j >> 3)
        if x > x1 or y > y1:
            continue
        m = min(int(budget[y, x]), max_samples)
        m_r = min(max(m - rnd * LW, 0), LW)
        out += [(slot << 3) | k for k in range(m_r)]
    return np.array(out, dtype=np.uint32)


def host_plan(H, w, h, rect, budget, max_samples, rnd, cap=None):
    x0, y0, x1, y1 = rect
    cap = ((x1 - x0 + 8) // 8) * ((y1 - y0 + 8) // 8) * 64 * LW if cap is None else cap
    lst = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    n = C.c_uint32(0)
    rc = H.lib().pt_test_film_plan_host(w, h, C.byref(H.PtRect(*rect)), budget.ctypes.data_as(H._up), max_samples, rnd, lst.ctypes.data_as(H._up), cap, C.byref(n))
    assert rc == H.OK, rc
    return lst[:min(n.value, cap)], n.value, lst


RECTS = [(0, 0, 66, 36), (9, 5, 40, 30), (33, 17, 33, 17), (8, 8, 15, 15), (60, 30, 66, 36)]  # the film; no edge on a tile boundary; one pixel; one whole tile; a corner


@pytest.mark.parametrize("rect", RECTS)
@pytest.mark.parametrize("rnd", [0, 1, 2])
@pytest.mark.parametrize("max_samples", [17, 9, 5, 4096])
def test_the_list_is_numpys_enumeration(H, rect, rnd, max_samples):
    w, h = 67, 37
    budget = BUDGETS[np.random.default_rng(3).integers(0, len(BUDGETS), size=(h, w))]
    want = numpy_plan(w, h, rect, budget, max_samples, rnd)
    got, n, _ = host_plan(H, w, h, rect, budget, max_samples, rnd)
    assert n == len(want) and np.array_equal(got, want)
    x0, y0, x1, y1 = rect
    inside = np.minimum(budget[y0:y1 + 1, x0:x1 + 1], max_samples).astype(np.int64)
    assert n == int(np.clip(inside - rnd * LW, 0, LW).sum()), "the length is the sum of m_r over the slice"
    assert np.all(np.diff(got.astype(np.int64)) > 0), "ascending (slot, j), every (slot, j) once"
    if rnd == 0 and rect == RECTS[0] and max_samples == 17:
        assert n > 0 and len(np.unique(got >> 3)) == int((inside > 0).sum())


def test_the_rounds_together_give_every_pixel_its_samples(H):
    w, h, rect = 67, 37, (9, 5, 40, 30)
    budget = BUDGETS[np.random.default_rng(4).integers(0, len(BUDGETS), size=(h, w))]
    per_slot = {}
    for rnd in range(4):
        got, n, _ = host_plan(H, w, h, rect, budget, 9, rnd)
        assert (n == 0) == (rnd >= 2)
        for e in got:
            per_slot[int(e) >> 3] = per_slot.get(int(e) >> 3, 0) + 1
    x0, y0, x1, y1 = rect
    tiles_x = (x1 - x0 + 8) // 8
    counts = np.zeros((h, w), dtype=np.uint32)
    for slot, k in per_slot.items():
        tile, j = slot >> 6, slot & 63
        counts[y0 + (tile // tiles_x) * 8 + (j >> 3), x0 + (tile % tiles_x) * 8 + (j & 7)] = k
    want = np.zeros((h, w), dtype=np.uint32)
    want[y0:y1 + 1, x0:x1 + 1] = np.minimum(budget[y0:y1 + 1, x0:x1 + 1], 9)
    assert np.array_equal(counts, want)


def test_a_short_buffer_and_bad_requests(H):
    lib = H.lib()
    w, h, rect = 67, 37, (0, 0, 66, 36)
    budget = np.full((h, w), 3, dtype=np.uint32)
    got, n, lst = host_plan(H, w, h, rect, budget, 8, 0, cap=10)
    assert n == 3 * w * h and len(got) == 10 and np.array_equal(got, numpy_plan(w, h, rect, budget, 8, 0)[:10])
    zeros = np.zeros((h, w), dtype=np.uint32)
    assert host_plan(H, w, h, rect, zeros, 8, 0)[1] == 0
    up = lambda a: a.ctypes.data_as(H._up)
    nn = C.c_uint32(7)
    r = H.PtRect(*rect)
    call = lambda *a: lib.pt_test_film_plan_host(*a)
    assert call(w, h, None, up(budget), 8, 0, up(lst), 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), None, 8, 0, up(lst), 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), up(budget), 8, 0, None, 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), up(budget), 8, 0, up(lst), 10, None) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), up(budget), 0, 0, up(lst), 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), up(budget), 4097, 0, up(lst), 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(r), up(budget), 8, 512, up(lst), 10, C.byref(nn)) == H.ERR_ARGUMENT
    assert call(w, h, C.byref(H.PtRect(0, 0, w, 0)), up(budget), 8, 0, up(lst), 10, C.byref(nn)) == H.ERR_SLICE
    assert call(w, h, C.byref(H.PtRect(3, 3, 2, 3)), up(budget), 8, 0, up(lst), 10, C.byref(nn)) == H.ERR_SLICE
    assert nn.value == 7
