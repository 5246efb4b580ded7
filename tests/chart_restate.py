"""The chart pass's contract (portrayer_amd/csrc/pt_chart.h, steps 1 to 10) restated in numpy float64, operation for operation, from the header's comments -
not from its code. Every numpy operation used here (+, -, *, /, sqrt on float64 arrays) is correctly rounded and nothing is fused, so this is a third reading
of the contract beside the kernels and the host replay (pt_test_chart_host), and the tests compare them bit for bit.

    chart(fwd, nrm, tri_v, tri_n, uv, width, height, flags=0) -> {"position": (H, W, 3) f64, "normal": (H, W, 3) f64, "tri": (H, W) i32, "covered": (H, W) u8}

fwd: the node's 12 doubles (rows 0..2 of its composed trans), nrm: its 9 (the upper 3x3 of its composed normal_trans); tri_v: (T, 9) corners a, b, c;
tri_n: (T, 9) vertex normals, or None where the node shades flat; uv: (T, 6), (u, v) of a, b, c. canonical=False evaluates every edge from its own first
endpoint instead of the canonically ordered pair: NOT the contract, the watertightness test's guard."""
import numpy as np

FLIP_NORMAL = 1
LIMIT = 16777216.0  # 2^24
CHUNK = 128         # triangles evaluated against all texels at a time


def corners(uv, width, height):
    """Steps 1 and 2: (T, 6) texel-space corners and which triangles take part."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 6)
    st = np.empty_like(uv)
    with np.errstate(all="ignore"):
        st[:, 0::2] = uv[:, 0::2] * float(width)
        st[:, 1::2] = (1.0 - uv[:, 1::2]) * float(height)
        part = np.all(np.abs(st) <= LIMIT, axis=1)  # (false for NaN and inf)
    return st, part


def edge(Ps, Pt, Qs, Qt, ps, pt, canonical=True):
    """Step 4: the value at p of the edge that runs from P to Q."""
    with np.errstate(all="ignore"):
        if not canonical:
            return (Qs - Ps) * (pt - Pt) - (Qt - Pt) * (ps - Ps)
        first = (Ps < Qs) | ((Ps == Qs) & (Pt <= Qt))
        Ls, Lt = np.where(first, Ps, Qs), np.where(first, Pt, Qt)
        Ms, Mt = np.where(first, Qs, Ps), np.where(first, Qt, Pt)
        E = (Ms - Ls) * (pt - Lt) - (Mt - Lt) * (ps - Ls)
        return np.where(first, E, -E)


def orientation(st, canonical=True):
    """Step 5: o per triangle and whether the triangle has an area."""
    area2 = edge(st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], st[:, 5], canonical)
    with np.errstate(all="ignore"):
        return np.where(area2 > 0.0, 1.0, -1.0), (area2 > 0.0) | (area2 < 0.0)


def weights(st, o, ps, pt, canonical=True):
    """Steps 6 and 7 for triangles st (c, 6) at points ps, pt (n,): w_a, w_b, w_c, sum and covers, each (c, n)."""
    c = [st[:, k][:, None] for k in range(6)]
    o = o[:, None]
    ps, pt = ps[None, :], pt[None, :]
    with np.errstate(all="ignore"):
        wc = o * edge(c[0], c[1], c[2], c[3], ps, pt, canonical)
        wa = o * edge(c[2], c[3], c[4], c[5], ps, pt, canonical)
        wb = o * edge(c[4], c[5], c[0], c[1], ps, pt, canonical)
        total = (wa + wb) + wc
        covers = (wa >= 0.0) & (wb >= 0.0) & (wc >= 0.0) & (total > 0.0)
    return wa, wb, wc, total, covers


def centres(width, height):
    q = np.arange(width * height)
    return (q % width).astype(np.float64) + 0.5, (q // width).astype(np.float64) + 0.5


def coverage(uv, width, height, canonical=True):
    """Steps 1 to 8: the owner per texel (-1: none) and how many triangles cover it, both (H * W,)."""
    st, part = corners(uv, width, height)
    o, has_area = orientation(st, canonical)
    live = np.nonzero(part & has_area)[0]
    ps, pt = centres(width, height)
    owner = np.full(width * height, -1, dtype=np.int64)
    count = np.zeros(width * height, dtype=np.int64)
    for k in range(0, len(live), CHUNK):
        ids = live[k:k + CHUNK]  # ascending
        cov = weights(st[ids], o[ids], ps, pt, canonical)[4]
        count += cov.sum(axis=0)
        anyc = cov.any(axis=0)
        firstc = ids[np.argmax(cov, axis=0)]
        take = anyc & (owner < 0)
        owner[take] = firstc[take]
    return owner, count


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def chart(fwd, nrm, tri_v, tri_n, uv, width, height, flags=0):
    fwd, nrm = np.asarray(fwd, dtype=np.float64).reshape(12), np.asarray(nrm, dtype=np.float64).reshape(9)
    tri_v = np.asarray(tri_v, dtype=np.float64).reshape(-1, 9)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 6)
    n = width * height
    owner, _ = coverage(uv, width, height)
    position, normal = np.zeros((n, 3)), np.zeros((n, 3))
    q = np.nonzero(owner >= 0)[0]
    if len(q):
        t = owner[q]
        st, _ = corners(uv[t], width, height)
        o, _ = orientation(st)
        ps, pt = centres(width, height)
        ps, pt = ps[q], pt[q]
        with np.errstate(all="ignore"):
            wc = o * edge(st[:, 0], st[:, 1], st[:, 2], st[:, 3], ps, pt)
            wa = o * edge(st[:, 2], st[:, 3], st[:, 4], st[:, 5], ps, pt)
            wb = o * edge(st[:, 4], st[:, 5], st[:, 0], st[:, 1], ps, pt)
            total = (wa + wb) + wc
            # step 9
            beta, gamma = wb / total, wc / total
            alpha = (1.0 - beta) - gamma
            v = tri_v[t]
            A, B, Cc = v[:, 0:3], v[:, 3:6], v[:, 6:9]
            p = (A * alpha[:, None] + B * beta[:, None]) + Cc * gamma[:, None]
            if tri_n is not None:
                vn = np.asarray(tri_n, dtype=np.float64).reshape(-1, 9)[t]
                m = (vn[:, 0:3] * alpha[:, None] + vn[:, 3:6] * beta[:, None]) + vn[:, 6:9] * gamma[:, None]
            else:
                e1, e2 = B - A, Cc - A
                m = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
            # step 10
            P = np.stack([((fwd[4 * r] * p[:, 0] + fwd[4 * r + 1] * p[:, 1]) + fwd[4 * r + 2] * p[:, 2]) + fwd[4 * r + 3] for r in range(3)], axis=1)
            Nw = np.stack([(nrm[3 * r] * m[:, 0] + nrm[3 * r + 1] * m[:, 1]) + nrm[3 * r + 2] * m[:, 2] for r in range(3)], axis=1)
            length = np.sqrt(_dot(Nw[:, 0], Nw[:, 1], Nw[:, 2], Nw[:, 0], Nw[:, 1], Nw[:, 2]))
            N = Nw / length[:, None]
            if flags & FLIP_NORMAL:
                N = -N
        position[q], normal[q] = P, N
    return {"position": position.reshape(height, width, 3), "normal": normal.reshape(height, width, 3),
            "tri": owner.astype(np.int32).reshape(height, width), "covered": (owner >= 0).astype(np.uint8).reshape(height, width)}


def min_weight_ratio(uv, width, height, owner):
    """Per texel the owner's smallest weight over its sum (0 where unowned): the cross-check's 'well inside' measure."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 6)
    own = np.asarray(owner).reshape(-1)
    out = np.zeros(own.shape)
    q = np.nonzero(own >= 0)[0]
    if len(q):
        st, _ = corners(uv[own[q]], width, height)
        o, _ = orientation(st)
        ps, pt = centres(width, height)
        ps, pt = ps[q], pt[q]
        wc = o * edge(st[:, 0], st[:, 1], st[:, 2], st[:, 3], ps, pt)
        wa = o * edge(st[:, 2], st[:, 3], st[:, 4], st[:, 5], ps, pt)
        wb = o * edge(st[:, 4], st[:, 5], st[:, 0], st[:, 1], ps, pt)
        out[q] = np.minimum(np.minimum(wa, wb), wc) / ((wa + wb) + wc)
    return out.reshape(np.asarray(owner).shape)


def host(lib, H, fwd, nrm, tri_v, tri_n, uv, width, height, flags=0):
    """pt_test_chart_host through ctypes, in chart()'s shapes."""
    import ctypes as C
    fwd, nrm = np.ascontiguousarray(fwd, dtype=np.float64).reshape(12), np.ascontiguousarray(nrm, dtype=np.float64).reshape(9)
    tri_v = np.ascontiguousarray(tri_v, dtype=np.float64).reshape(-1, 9)
    tn = None if tri_n is None else np.ascontiguousarray(tri_n, dtype=np.float64).reshape(-1, 9)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 6)
    out = {"position": np.full((height, width, 3), 7.0), "normal": np.full((height, width, 3), 7.0), "tri": np.full((height, width), 7, dtype=np.int32),
           "covered": np.full((height, width), 7, dtype=np.uint8)}
    b = H.PtChartBuffers(H._p(out["position"], H._dp), H._p(out["normal"], H._dp), H._p(out["tri"], H._ip), H._p(out["covered"], H._u8p))
    rc = lib.pt_test_chart_host(H._p(fwd, H._dp), H._p(nrm, H._dp), len(tri_v), H._p(tri_v, H._dp), H._p(tn, H._dp), H._p(uv, H._dp), width, height, flags, C.byref(b))
    assert rc == 0, rc
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the cases the CPU and the GPU tests share: name -> (tri_v (T, 9), tri_n (T, 9), uv (T, 6), width, height)
def _tri_from_uv(uv):
    """A surface over the unit square, so that a chart's points are easy to look at: (2u - 1, 2v - 1, a bump); normals that are not the faces'."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 3, 2)
    with np.errstate(all="ignore"):
        u, v = np.nan_to_num(uv[..., 0], nan=0.3, posinf=1.5, neginf=-1.5), np.nan_to_num(uv[..., 1], nan=0.6, posinf=1.5, neginf=-1.5)
        u, v = np.clip(u, -4.0, 4.0), np.clip(v, -4.0, 4.0)
    pos = np.stack([2.0 * u - 1.0, 2.0 * v - 1.0, 0.25 * np.sin(3.0 * u) * np.cos(2.0 * v)], axis=-1)
    nrm = np.stack([0.3 * np.cos(3.0 * u), 0.2 * np.sin(2.0 * v), np.ones_like(u)], axis=-1)
    return pos.reshape(-1, 9), nrm.reshape(-1, 9)


def grid_uv(seed, width, height, cells=8, spread=0.1, snap=True):
    """cells x cells quads (two triangles each) over the exact unit square; interior UV vertices moved by random offsets below a third of a cell. The offsets are
    drawn below `spread` of a cell; with snap, every interior vertex is then moved to where two lines meet - from its left and from its lower neighbour, both placed already,
    each through the texel centre closest to that edge - so that both edges pass through a texel centre up to rounding, the only place where an edge
    function's sign is in doubt; it must stay within 0.3 of a cell of its lattice position, else it keeps its random offset. Returns (T, 6) per-corner UVs, T = 2 cells^2."""
    rng = np.random.default_rng(seed)
    g = np.zeros((cells + 1, cells + 1, 2))
    for j in range(cells + 1):
        for i in range(cells + 1):
            g[j, i] = (i / cells, j / cells)
    base = g.copy()
    g[1:cells, 1:cells] += rng.uniform(-spread, spread, size=(cells - 1, cells - 1, 2)) / cells
    if snap:
        W, Hh = float(width), float(height)

        def texel(c):
            return np.array([c[0] * W, (1.0 - c[1]) * Hh])

        def centre_near(Ls, Ms):
            """the texel centre closest to the line Ls -> Ms among those beside its middle half, or None"""
            d = Ms - Ls
            lo, hi = np.floor(np.minimum(Ls, Ms)) - 1, np.ceil(np.maximum(Ls, Ms)) + 1
            xs, ys = np.meshgrid(np.arange(lo[0], hi[0]) + 0.5, np.arange(lo[1], hi[1]) + 0.5)
            px, py = xs.ravel(), ys.ravel()
            along = ((px - Ls[0]) * d[0] + (py - Ls[1]) * d[1]) / (d @ d)
            off = np.abs((px - Ls[0]) * d[1] - (py - Ls[1]) * d[0]) / np.sqrt(d @ d)
            ok = (along > 0.25) & (along < 0.75)
            if not ok.any():
                return None
            k = np.argmin(np.where(ok, off, np.inf))
            return np.array([px[k], py[k]])

        for j in range(1, cells):
            for i in range(1, cells):
                L1, L2, M = texel(g[j, i - 1]), texel(g[j - 1, i]), texel(g[j, i])  # the left and the lower neighbour: placed already
                p1, p2 = centre_near(L1, M), centre_near(L2, M)
                if p1 is None or p2 is None:
                    continue
                d1, d2 = p1 - L1, p2 - L2
                den = d1[0] * d2[1] - d1[1] * d2[0]
                if den == 0.0:
                    continue
                new = L1 + d1 * (((L2 - L1)[0] * d2[1] - (L2 - L1)[1] * d2[0]) / den)  # where the lines L1 -> p1 and L2 -> p2 meet
                cand = np.array([new[0] / W, 1.0 - new[1] / Hh])
                if not np.all(np.abs(cand - base[j, i]) < 0.3 / cells):
                    continue
                g[j, i] = cand
                # ... and among the 7 x 7 doubles around it, one for which the two ways round the edge to the left neighbour disagree at p1: evaluated from
                # either endpoint, as a triangle's own order would, the edge function has the same strict sign on both sides (a gap, or a double cover)
                steps = [0, 1, -1, 2, -2, 3, -3]
                for a in steps:
                    for b in steps:
                        c = cand.copy()
                        for _ in range(abs(a)):
                            c[0] = np.nextafter(c[0], np.inf if a > 0 else -np.inf)
                        for _ in range(abs(b)):
                            c[1] = np.nextafter(c[1], np.inf if b > 0 else -np.inf)
                        Mm = texel(c)
                        e1 = (Mm[0] - L1[0]) * (p1[1] - L1[1]) - (Mm[1] - L1[1]) * (p1[0] - L1[0])
                        e2 = (L1[0] - Mm[0]) * (p1[1] - Mm[1]) - (L1[1] - Mm[1]) * (p1[0] - Mm[0])
                        if e1 * e2 > 0.0:
                            g[j, i] = c
                            break
                    else:
                        continue
                    break
    assert np.all(np.abs(g - base) < 1.0 / (3.0 * cells))
    uv = []
    for j in range(cells):
        for i in range(cells):
            v00, v10, v11, v01 = g[j, i], g[j, i + 1], g[j + 1, i + 1], g[j + 1, i]
            uv.append(np.concatenate([v00, v10, v11]))
            uv.append(np.concatenate([v00, v11, v01]))
    return np.array(uv)


def cases():
    """name -> (tri_v, tri_n, uv, [(width, height), ...])"""
    out = {}
    one = np.array([[0.1, 0.15, 0.9, 0.2, 0.45, 0.95]])
    out["one_triangle"] = (one, [(1, 1), (2, 2), (7, 5)])
    out["other_winding"] = (one.reshape(1, 3, 2)[:, ::-1].reshape(1, 6).copy(), [(7, 5)])
    out["quad_diagonal"] = (np.array([[0.0, 0.0, 1.0, 0.0, 1.0, 1.0], [0.0, 0.0, 1.0, 1.0, 0.0, 1.0]]), [(8, 8)])  # the diagonal runs through 8 centres
    good = [[0.05, 0.05, 0.5, 0.1, 0.1, 0.6], [0.5, 0.1, 0.95, 0.9, 0.1, 0.6]]
    bad = [[0.25, 0.25, 0.5, 0.5, 0.75, 0.75],                 # no area (dyadic: the corners are exact in texel space, and collinear)
           [0.2, float("nan"), 0.8, 0.3, 0.5, 0.9],            # a NaN
           [0.2, 0.1, float("inf"), 0.3, 0.5, 0.9],            # an inf
           [0.2, 0.1, 0.8, 0.3, 2.0 ** 25, 0.9]]               # beyond 2^24 texels at every size used
    out["bad_among_good"] = (np.array([bad[0], good[0], bad[1], bad[2], good[1], bad[3]]), [(7, 5), (64, 64)])
    out["good_alone"] = (np.array(good), [(7, 5), (64, 64)])
    out["outside_unit"] = (np.array([[-0.4, -0.3, 1.6, 0.2, 0.3, 1.7], [0.5, 0.5, 2.5, 0.6, 2.0, 3.0], [-3.0, -3.0, -2.0, -3.0, -2.0, -2.0]]), [(7, 5), (67, 37)])
    out["overlap"] = (np.array([[0.3, 0.3, 0.9, 0.35, 0.5, 0.9], [0.1, 0.1, 0.8, 0.15, 0.4, 0.8], [0.2, 0.05, 0.95, 0.5, 0.3, 0.7]]), [(64, 64), (67, 37)])
    out["grid"] = (grid_uv(3, 64, 64), [(64, 64), (67, 37)])
    full = {}
    for name, (uv, sizes) in out.items():
        v, n = _tri_from_uv(uv)
        full[name] = (v, n, uv, sizes)
    return full


def node_matrices():
    """A rotated, non-uniformly scaled and translated node: (fwd 12, nrm 9) with nrm the inverse transpose of fwd's 3x3; and the identity's."""
    a, b = 0.7, -0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    m = rz @ rx @ np.diag([1.5, 0.6, 2.25])
    fwd = np.concatenate([m, np.array([[0.3], [-1.2], [2.0]])], axis=1).reshape(12)
    nrm = np.linalg.inv(m).T.reshape(9)
    ident = (np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).reshape(12), np.eye(3).reshape(9))
    return (fwd, nrm), ident
