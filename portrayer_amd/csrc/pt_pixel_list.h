// Per-pixel candidate lists for primary rays: which leaves of the scene tree ANY ray from the eye through one pixel's square can reach.
//
// A wavefront of the headline launch holds the 64 samples of one pixel, and which leaves their rays reach is a property of the pixel: in front of the launch
// pt_pixel_list_kernel (pt_api.hip) walks sc.bvh once per PIXEL with the pixel's BEAM - per axis the range of the rays' directions over the square - and stores
// the leaves whose boxes the beam reaches, nearest first. The render kernel's primary stage (pt_render_simple.h) runs the walk's own leaf test on that list
// and skips the walk; a pixel with no candidate is background without a ray. The tree only ever culled: the result is the nearest candidate, the lowest index
// on exact ties (pt_cand_end), whatever is tested in whatever order - a change of schedule, like the occluder table.
//
// THE OBLIGATION. Whenever the walk's slab test (pt_slab_pk2 with pt_raypk's constants, any octant form, any bound up to +inf) accepts a box for the ray of a
// sample position in [x, x + 1] x [y, y + 1], pt_beam_box accepts that box for pixel (x, y). The walk's test is itself wider than the exact one, so this is
// more than geometric conservatism: the beam's margins must dominate the walk's.
//
// 1. The beam. pt_camera_ray gives a sample at (sx, sy) the direction d = D / |D|, D = world(sx, sy) - eye, where every operation up to D is a division or product
//    by a constant, or a sum: each is monotone (weakly) in sx and in sy IN FLOATING POINT (rounding is monotone), so over the square every component of the
//    computed D lies between its values at the four corners, computed by the same expressions (pt_beam_corner repeats pt_camera_ray's, under the same
//    -ffp-contract=off). sx = (double)x + jx with jx in [0, 1) rounds into [x, x + 1]. The normalisation then costs d_a = (D_a / L)(1 + 3e-16), L = |D|.
// 2. The walk's values. For a plane P of axis a (an f32) and a unit direction d the walk computes (pt_raypk_axis_f32, its derivation, with T = (P - o) / d_a exact,
//    u = 2^-24, w <= 2.41e-7 |o / d_a| + 2e-20 (1 + u)):   v = fma(P, i, c),  i = (1 / d_a)(1 + e1), |e1| < 2^-20.3 (2^-22.4 from the reciprocal - the device's is one
//    ulp off, the host's is rounded -, 2^-21 (1 + u) of deliberate bias, one rounding),  |c + o i| <= 2 w (w itself, the origin's conversion and the fma's rounding,
//    which w was sized to cover), and one last rounding u |v|:     |v - T| <= 2^-20.1 |T| + 2.01 w + 2^-126.
//    The entering value of an axis is one of the two planes' values (which one depends on the octant form; the mixed form takes the smaller), the leaving value
//    the other; the walk accepts iff max(entering values, 0) <= min(leaving values, bound).
// 3. Scale. Acceptance compares parameters of ONE ray with each other and with 0, so dividing all of them by L > 0 changes nothing: v / L against
//    T / L = (P - o) / D_a, with the margin 2^-20.1 |(P - o) / D_a| + 2.01 (2.41e-7 |o / D_a| + 2e-20 / L) + 2^-126 / L. The beam test works in these units and
//    never normalises.
// 4. The beam test: per pixel the constants in f64 (pt_beam_setup, once), per box 12 f32 fmas and the min / max around them (pt_beam_box). Per axis with D_a in [Dl, Dh], Dl > 0 (a negative range is mirrored:
//    planes, origin and range change sign; the mirror is folded into the constants' signs and into which plane feeds which fma), n_lo = P_lo - o, n_hi = P_hi - o,
//    the target is, from 3. and with every |o / D_a| <= |o| / Dl,
//        E <= min over [Dl, Dh] of (n_lo - 2^-20.1 |n_lo|) / D_a  - M,      F >= max over [Dl, Dh] of (n_hi + 2^-20.1 |n_hi|) / D_a  + M,
//        M = 4.85e-7 |o| / Dl + 4.1e-20 / Lmin.
//    Constants: A1 = f32(1 / Dh (1 - 2^-18)) <= (1 / Dh)(1 - 2^-18.1), A2 = f32(1 / Dl (1 + 2^-18)) >= (1 / Dl)(1 + 2^-18.1) (the conversion's 2^-24 and the division's
//    2^-53 are inside the step from 2^-18 to 2^-18.1), m = 6e-7 |o| / Dl + 5e-20 / Lmin + 1e-12 (|o| A2) >= M (1 + 2^-22) + the f64 roundings of what follows,
//    Be_k = the f32 at or below -o A_k - m, Bf_k = the f32 at or above -o A_k + m (A_k as the f32 it is; the f64 product and sum rounded once more, outward). Then
//        E = min(fma(P_lo, A1, Be_1), fma(P_lo, A2, Be_2)),      F = max(fma(P_hi, A1, Bf_1), fma(P_hi, A2, Bf_2)).
//    For n_lo >= 0: the first fma is, before its one rounding, at most n_lo A1 - m, and after it at most n_lo A1 (1 + 2^-24) - m (1 - 2^-24)
//    <= n_lo (1 / Dh)(1 - 2^-18.1 + 2^-24) - M - where 2^-18.1 - 2^-24 > 2^-20.1, and (n_lo - 2^-20.1 n_lo) / D_a is smallest at Dh. For n_lo < 0 the second is at most
//    n_lo A2 (1 - 2^-24) - m (1 - 2^-24) <= n_lo (1 / Dl)(1 + 2^-20.1) - M, the target's value at Dl. The minimum of the two is below whichever applies. F likewise
//    with the roles exchanged. (Where the cancellation in P A + B loses digits - an eye far from the origin - the loss is 2^-24 of |o A|, a tenth of m: the walk's own f32
//    planes and origin have the same problem and w is its answer there.) n -> n -+ 2^-20.1 |n| is increasing, so E lies below BOTH planes' walk values of every sample and
//    F above both: whichever of them an octant form calls entering, E <= entering / L and leaving / L <= F for every sample of the pixel. Accepted unless
//    max(E_x, E_y, E_z, 0) > min(F_x, F_y, F_z): if the walk accepts the box for sample s with parameter t, then t / L(s) lies in every axis' [E, F] and is >= 0.
//    The comparison is written so that a NaN accepts; fmaxf / fminf drop a NaN operand, as v_max / v_min do in the walk. An axis whose constants are not finite, or with
//    A2 > 1e19 (|P| <= 1e18, pt_scene_upload: every product stays below FLT_MAX), constrains nothing (5.).
// 5. Axes whose range reaches zero. The walk switches an axis off - entering -inf, leaving +inf, whatever the origin - where |rcp((float)d_a)| > 1e18, i.e.
//    |D_a| < 1.0001e-18 L. An axis with Dl <= 4e-18 Lmax and Dh >= -4e-18 Lmax (Lmax >= L from the ranges' largest magnitudes) has no E and no F: it contains every
//    such sample, and every sample pair of opposite signs. A NaN in a range does the same.
// 6. The bound stored with an accepted box: every sample ray's entry parameter into the box, for its unit direction, is t_in >= max(entering values, 0) in the
//    walk's arithmetic and likewise exactly (E lies below the exact (P - o) / D_a of the entering plane as well), so t_in >= max(E_x, E_y, E_z, 0) L >= Emax Lmin,
//    Lmin^2 = the sum of the ranges' smallest squared magnitudes. Stored as the f32 below it, of which the record keeps the upper 16 bits (truncation of a positive float
//    rounds toward zero). A hit of the leaf's primitive lies inside the box at t >= t_in up to f64 rounding (2^-52), five orders of magnitude inside the 2^-19 the bound gave away.
// 7. Any rectangle. Nothing in 1. to 6. uses the square's size: for sample positions in [px, px + nx] x [py, py + ny] (nx, ny >= 0) the computed D still lies between its
//    values at the rectangle's four corners (1.: monotone rounding), Lmin and Lmax still come from the ranges, and 2. to 6. speak of one sample's ray against ranges that
//    contain it. So pt_beam_setup(c, px, py, nx, ny) owes the same: whatever the walk accepts for a sample position inside the rectangle, pt_beam_box accepts, and the bound
//    lies below every such ray's entry parameter. The pixel's beam is nx = ny = 1 (px + 1.0 as before: the same bits). The list kernel's TILE beam is the 8 x 8 rectangle of
//    a tile's 64 pixel slots, from lane 0's pixel: a box that any pixel's sample ray reaches in the walk is accepted by it, so every ancestor of a leaf that is hit gets
//    opened. What does NOT follow, and is not needed: that a box the pixel's beam accepts is accepted by the tile's - the two sets of f32 constants are rounded
//    independently, so a box that grazes the pixel's beam (and that no ray hits) may be turned away by the tile's.
#pragma once

#include "pt_scene_view.h"

// A pixel's record: 8 words = 32 bytes, half a line. K = 6 from the counting build's figures (profiles/r12/notes.md section 1: a list cut at 6 entries sends 0.43 % of
// big-scene's items to the walk, one cut at 14 0.13 %, and the record is half the size).
//   word 0   bits 0..7 the number of entries n <= PT_PL_K; bit 31 (PT_PL_WALK): unusable, take the walk
//   word 1   the tail bound as an f32: the smallest bound among the accepted leaves' nodes NOT in the list (+inf: none was left out)
//   word 2+k entry k: bound's upper 16 bits << 16 | flattened node index (< 65536: the host leaves the lists out for larger scenes). Ascending as unsigned words, which is
//            ascending in the bound (non-negative floats order like their bit patterns), then in the index.
// In front of the records one 64-byte header, behind the launch's eye table and certain-shadow table (pt_pl_header): word 0 != 0: the records follow; 0: no lists, today's walk.
// Word 0 bit 1 (PT_PL_QUEUE): behind the records the launch's QUEUE follows, one word per pixel slot - the slot ids (local tile << 6 | j) of the pixels that need the render
// kernel, i.e. the in-slice slots whose record is not {0 entries, infinite tail, unmarked} - and header word 1 holds their number. The host zeroes the header, the list kernel
// writes word 0 and a 64-bit mask per tile behind the queue, and pt_pixel_queue_kernel (pt_api.hip) makes the queue and word 1 of the masks: the tiles' ranges in the order of
// the tiles, a tile's ids in the Morton order the render kernel deals a tile's pixels in (pt_tile_order_to_slot) - the order in which the pixels were dealt without a queue,
// which the occluder table's look at the tile above was measured to need (profiles/r15/notes.md). The render kernel deals only queued pixels; the finish kernel
// finishes the others from the background alone (pt_background_sum). PORTRAYER_BACKGROUND_SKIP=0, -DPT_NO_BACKGROUND_SKIP: no queue, every pixel dealt.
#ifndef PT_PL_K  // (-DPT_PL_K=14u with -DPT_PIXEL_LIST_STATS: the build the figures were taken from - 16-word records, so that caps up to 14 can be tried)
#define PT_PL_K 6u
#endif
#define PT_PL_WORDS (PT_PL_K <= 6u ? 8u : 16u)
static_assert(PT_PL_K >= 1u && PT_PL_K <= 14u, "a record is 8 or 16 words: head, tail bound, entries");
#define PT_PL_WALK 0x80000000u
#define PT_PL_MAX_NODES 65536u
#define PT_PL_INF_BITS 0x7F800000u

// where the header lies behind an eye table of n_nodes records (96 + 16 bytes each), as a byte offset: the next multiple of 64
PT_HD size_t pt_pl_header_offset(uint32_t n_nodes) { return ((size_t)n_nodes * (12 * sizeof(double) + 4 * sizeof(float)) + 63u) & ~(size_t)63u; }
// (with the queue: a word per slot for it, and behind it the 64-bit mask per tile it is made from - n_slots is a multiple of 64, so the masks are 8-byte aligned)
PT_HD size_t pt_pl_bytes(uint32_t n_slots, bool queue = false) { return 64u + (size_t)n_slots * (PT_PL_WORDS * 4u) + (queue ? (size_t)n_slots * 4u + (size_t)(n_slots / 64u) * 8u : 0u); }
// the tiles' masks, from the first record's address
PT_HD unsigned long long* pt_pl_masks(uint32_t* records, uint32_t n_slots) { return reinterpret_cast<unsigned long long*>(records + (size_t)n_slots * (PT_PL_WORDS + 1u)); }
#define PT_PL_LISTS 1u  // header word 0: the records follow
#define PT_PL_QUEUE 2u  // header word 0: ... and the queue behind them, its length in header word 1
// the inverse of pt_tile_order_to_slot: j = y * 8 + x inside the 8x8 tile -> its place in the tile's Morton order
PT_HD uint32_t pt_pl_slot_to_tile_order(uint32_t j) {
    return (j & 1u) | ((j >> 2) & 2u) | ((j << 1) & 4u) | ((j >> 1) & 8u) | ((j << 2) & 16u) | (j & 32u);
}

struct PtBeamAxis {
    int neg;             // 1: every sample's direction is negative on this axis - the box's UPPER plane feeds the entering fmas, the lower one the leaving fmas
    float a1, a2;        // A1, A2 of 4. (the mirror folded in: negated where neg); 0 on an axis that constrains nothing (5.)
    float be1, be2;      // Be_1, Be_2;  -inf on such an axis
    float bf1, bf2;      // Bf_1, Bf_2;  +inf on such an axis
};
struct PtBeam {
    PtBeamAxis ax[3];
    float lmin;  // an f32 below Lmin (6.)
};

// the f32 at or below v / at or above v (v finite or not; a NaN stays one)
PT_HD float pt_f32_below(double v) {
    float f = (float)v;
    if ((double)f > v) {
        const uint32_t u = __builtin_bit_cast(uint32_t, f);
        f = f > 0.0f ? __builtin_bit_cast(float, u - 1u) : (f < 0.0f ? __builtin_bit_cast(float, u + 1u) : -1.401298464324817e-45f);
    }
    return f;
}
PT_HD float pt_f32_above(double v) { return -pt_f32_below(-v); }

// pt_camera_ray's expressions up to the subtraction of the eye (pt_shade.h; camera.rs:48-84), in two steps: the view coordinate of a sample coordinate - two of
// each per pixel, shared by the corners - and the corner's direction from the two
PT_HD double pt_beam_view_x(const PtCamera& c, double x) {
    double ndc_x = x / c.width;
    return (2.0 * ndc_x - 1.0) * c.aspect * c.fov_factor;
}
PT_HD double pt_beam_view_y(const PtCamera& c, double y) {
    double ndc_y = y / c.height;
    return (1.0 - 2.0 * ndc_y) * c.fov_factor;
}
PT_HD void pt_beam_corner(const PtCamera& c, double view_x, double view_y, double D[3]) {
    PtVec3 eye = pt_v3(c.eye[0], c.eye[1], c.eye[2]);
    PtVec3 world = pt_xform_point(c.view_to_world, pt_v3(view_x, view_y, -1.0));
    PtVec3 d = world - eye;
    D[0] = d.x; D[1] = d.y; D[2] = d.z;
}

// The beam of the sample positions in [px, px + nx] x [py, py + ny] (7.); a pixel's: nx = ny = 1, every sample position in [px, px + 1] x [py, py + 1].
PT_HD PtBeam pt_beam_setup(const PtCamera& c, double px, double py, double nx = 1.0, double ny = 1.0) {
    double lo[3], hi[3];
    bool finite = true;  // (a NaN or an infinity in a corner: no axis constrains anything)
    const double vx[2] = {pt_beam_view_x(c, px), pt_beam_view_x(c, px + nx)}, vy[2] = {pt_beam_view_y(c, py), pt_beam_view_y(c, py + ny)};
    for (int k = 0; k < 4; k++) {
        double D[3];
        pt_beam_corner(c, vx[k & 1], vy[k >> 1], D);
        for (int a = 0; a < 3; a++) {
            finite = finite && fabs(D[a]) < INFINITY;
            if (k == 0) { lo[a] = hi[a] = D[a]; }
            else { lo[a] = fmin(lo[a], D[a]); hi[a] = fmax(hi[a], D[a]); }
        }
    }
    double lmax2 = 0.0, lmin2 = 0.0;
    for (int a = 0; a < 3; a++) {
        const double m = fmax(fabs(lo[a]), fabs(hi[a]));
        lmax2 += m * m;
        const double n = (lo[a] > 0.0) ? lo[a] : ((hi[a] < 0.0) ? -hi[a] : 0.0);
        lmin2 += n * n;
    }
    const double lmax = sqrt(lmax2) * (1.0 + 1e-12), lmin = sqrt(lmin2) * (1.0 - 1e-12);
    const double zt = 4e-18 * lmax;
    const double c0 = lmin > 0.0 ? 5e-20 / lmin : (double)INFINITY;
    PtBeam b;
    for (int a = 0; a < 3; a++) {
        PtBeamAxis& x = b.ax[a];
        x.neg = 0; x.a1 = x.a2 = 0.0f; x.be1 = x.be2 = -INFINITY; x.bf1 = x.bf2 = INFINITY;
        double dl, dh, o;
        if (!finite) continue;
        if (lo[a] > zt && hi[a] >= lo[a]) { o = c.eye[a]; dl = lo[a]; dh = hi[a]; }
        else if (hi[a] < -zt && hi[a] >= lo[a]) { x.neg = 1; o = -c.eye[a]; dl = -hi[a]; dh = -lo[a]; }
        else continue;
        const float a1 = (float)((1.0 / dh) * (1.0 - 0x1p-18)), a2 = (float)((1.0 / dl) * (1.0 + 0x1p-18));
        const double m = (6e-7 * fabs(o)) * (double)a2 + c0 + 1e-12 * (fabs(o) * (double)a2);  // (a2 >= 1 / dl)
        const float be1 = pt_f32_below(-o * (double)a1 - m), be2 = pt_f32_below(-o * (double)a2 - m);
        const float bf1 = pt_f32_above(-o * (double)a1 + m), bf2 = pt_f32_above(-o * (double)a2 + m);
        // (constants that are not finite, a zero or a huge multiplier: the axis constrains nothing - a comparison with a NaN is false)
        if (!(a1 > 0.0f && a2 <= 1e19f && fabsf(be1) < INFINITY && fabsf(be2) < INFINITY && fabsf(bf1) < INFINITY && fabsf(bf2) < INFINITY)) { x.neg = 0; continue; }
        x.a1 = x.neg ? -a1 : a1; x.a2 = x.neg ? -a2 : a2;
        x.be1 = be1; x.be2 = be2; x.bf1 = bf1; x.bf2 = bf2;
    }
    const float lm = (float)(lmin * (1.0 - 1e-6));
    b.lmin = lm > 0.0f && lm < INFINITY ? lm : 0.0f;
    return b;
}

// One box (f32 planes, as the tree holds them) against the beam. *bound (where accepted): an f32 at or below the lower bound of 6.
PT_HD bool pt_beam_box(const PtBeam& b, const float lo[3], const float hi[3], float* bound) {
    float en = 0.0f, lv = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const PtBeamAxis& x = b.ax[a];
        const float pe = x.neg ? hi[a] : lo[a], pf = x.neg ? lo[a] : hi[a];
        const float e = fminf(__builtin_fmaf(pe, x.a1, x.be1), __builtin_fmaf(pe, x.a2, x.be2));
        const float f = fmaxf(__builtin_fmaf(pf, x.a1, x.bf1), __builtin_fmaf(pf, x.a2, x.bf2));
        en = fmaxf(en, e);  // (a NaN - an infinite plane, an axis without constants - is dropped: no constraint from it)
        lv = fminf(lv, f);
    }
    if (en > lv) return false;
    float fb = (en * b.lmin) * (1.0f - 0x1p-22f);  // (the product's and this one's rounding, and more)
    if (!(fb >= 0.0f)) fb = 0.0f;
    *bound = fb;
    return true;
}

// an entry word and back
PT_HD uint32_t pt_pl_entry(float bound, uint32_t node) { return (__builtin_bit_cast(uint32_t, bound) & 0xFFFF0000u) | (node & 0xFFFFu); }
PT_HD float pt_pl_entry_bound(uint32_t e) { return __builtin_bit_cast(float, e & 0xFFFF0000u); }
PT_HD uint32_t pt_pl_entry_node(uint32_t e) { return e & 0xFFFFu; }

// One pixel's list while it is built: `list` = its K words, `stride` words apart (a lane's LDS column; 1 on the host). Keeps the `cap` smallest entries in
// ascending order and the smallest bound of what it turns away in *tail (as f32 bits; PT_PL_INF_BITS: nothing yet). cap <= PT_PL_K.
PT_HD void pt_pl_insert(uint32_t* list, uint32_t stride, uint32_t cap, uint32_t* count, uint32_t* tail, uint32_t e) {
    uint32_t i;
    if (*count < cap) {
        i = (*count)++;
    } else {
        const uint32_t last = cap ? list[(cap - 1u) * stride] : 0u;
        const uint32_t out = (cap == 0u || e >= last) ? e : last;  // the one that does not fit
        const uint32_t ob = out & 0xFFFF0000u;
        if (ob < *tail) *tail = ob;
        if (cap == 0u || e >= last) return;
        i = cap - 1u;
    }
    while (i > 0u && list[(i - 1u) * stride] > e) { list[i * stride] = list[(i - 1u) * stride]; i--; }
    list[i * stride] = e;
}
