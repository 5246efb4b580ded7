// The contract of the chart pass (pt_chart, include/portrayer_hip.h): which surface point a texel of a mesh's light map is. A fixed sequence of
// correctly rounded f64 operations (+, -, *, /, sqrt; no fused multiply-add: the build passes -ffp-contract=off) as PT_HD functions - the kernels
// (pt_chart.hip) and the host replay (pt_test_chart_host) compile this very text, and tests/chart_restate.py restates it in numpy from these comments.
//
// Inputs: a flattened mesh node i with triangles t = 0 .. T - 1 (records tri_first + t of tri_v / tri_n), a UV set of T x 6 doubles - (u, v) of the corners
// a, b, c of every triangle - and a map of W x H texels.
//   1. texel space   a corner is s = u * W, t = (1 - v) * H (rows run top to bottom, triangle.rs:98). No wrap: what lies outside [0, 1] falls off the map.
//   2. takes part    all six of a triangle's s and t finite and at most 2^24 in magnitude; otherwise the triangle owns nothing.
//   3. sample        texel (x, y), index q = y W + x, is sampled at p = (x + 0.5, y + 0.5).
//   4. edge          for an edge with endpoints P, Q in this order: P comes first when P.s < Q.s, or P.s == Q.s and P.t <= Q.t. (L, M) = (P, Q) then, else (Q, P).
//                    E = (M.s - L.s) * (p.t - L.t) - (M.t - L.t) * (p.s - L.s): two products, one subtraction. The edge's value is E if (L, M) = (P, Q), else -E.
//                    Two triangles that share an edge with bit-equal endpoints compute the same E and give it opposite signs where they run through the edge in
//                    opposite directions: at least one of them accepts any p with respect to that edge.
//   5. area          area2 = edge (a, b) at c. o = +1 if area2 > 0, -1 if area2 < 0; area2 == 0 or NaN: the triangle owns nothing.
//   6. weights       w_c = o * edge(a, b)(p), w_a = o * edge(b, c)(p), w_b = o * edge(c, a)(p), sum = (w_a + w_b) + w_c.
//   7. covers        w_a >= 0 && w_b >= 0 && w_c >= 0 && sum > 0: inclusive, a centre exactly on a shared edge is covered by both neighbours.
//   8. owner         the LOWEST t that covers the texel, or none.
//   9. surface       beta = w_b / sum, gamma = w_c / sum, alpha = (1 - beta) - gamma (triangle.rs:84). Model point (A alpha + B beta) + C gamma per component.
//                    Model normal: (na alpha + nb beta) + nc gamma where the node shades smoothly, else pt_cross(B - A, C - A) (triangle.rs:82-88) - the choice
//                    pt_hit_model makes.
//  10. world         P = pt_xform_point(fwd + 12 i, p); N = pt_normalized(pt_xform_dir(nrm + 9 i, 3, n)), every component negated with PT_CHART_FLIP_NORMAL.
//                    fwd and nrm are the COMPOSED matrices in all three traversals. In the hierarchical semantics a render carries a hit up its path level by
//                    level (scene.rs:100-112) and rounds differently in the last bits: the pass defines surface points, not hits.
// An unowned texel reports position (0, 0, 0), normal (0, 0, 0), tri -1, covered 0: an invalid point for pt_ao and pt_gather (pt_ao_valid).
#pragma once

#include "pt_math.h"

#define PT_CHART_FLAG_FLIP_NORMAL 1u  // == PT_CHART_FLIP_NORMAL (include/portrayer_hip.h)
#define PT_CHART_LIMIT 16777216.0     // 2^24 (step 2)
#define PT_CHART_NONE 0xFFFFFFFFu     // the owner map's "nobody"

// Steps 1 and 2: uv = (u, v) of a, b, c; st = (s, t) of a, b, c. False: the triangle owns nothing.
PT_HD bool pt_chart_corners(const double uv[6], uint32_t W, uint32_t H, double st[6]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        st[2 * k] = uv[2 * k] * (double)W;
        st[2 * k + 1] = (1.0 - uv[2 * k + 1]) * (double)H;
        ok = ok && fabs(st[2 * k]) <= PT_CHART_LIMIT && fabs(st[2 * k + 1]) <= PT_CHART_LIMIT;  // (false for NaN and inf)
    }
    return ok;
}

// Step 4: the value at (ps, pt) of the edge that runs from P to Q.
PT_HD double pt_chart_edge(double Ps, double Pt, double Qs, double Qt, double ps, double pt) {
    const bool first = Ps < Qs || (Ps == Qs && Pt <= Qt);
    const double Ls = first ? Ps : Qs, Lt = first ? Pt : Qt, Ms = first ? Qs : Ps, Mt = first ? Qt : Pt;
    const double E = (Ms - Ls) * (pt - Lt) - (Mt - Lt) * (ps - Ls);
    return first ? E : -E;
}

// Step 5. False: the triangle owns nothing.
PT_HD bool pt_chart_orientation(const double st[6], double* o) {
    const double area2 = pt_chart_edge(st[0], st[1], st[2], st[3], st[4], st[5]);
    *o = area2 > 0.0 ? 1.0 : -1.0;
    return area2 > 0.0 || area2 < 0.0;
}

// Steps 6 and 7 at p = (ps, pt); w = {w_a, w_b, w_c, sum}.
PT_HD bool pt_chart_covers(const double st[6], double o, double ps, double pt, double w[4]) {
    w[2] = o * pt_chart_edge(st[0], st[1], st[2], st[3], ps, pt);
    w[0] = o * pt_chart_edge(st[2], st[3], st[4], st[5], ps, pt);
    w[1] = o * pt_chart_edge(st[4], st[5], st[0], st[1], ps, pt);
    w[3] = (w[0] + w[1]) + w[2];
    return w[0] >= 0.0 && w[1] >= 0.0 && w[2] >= 0.0 && w[3] > 0.0;
}

// Step 9: v = the triangle's 72-byte record of tri_v, vn = that of tri_n or null where the node shades flat.
PT_HD void pt_chart_surface(const double* v, const double* vn, const double w[4], PtVec3* p, PtVec3* n) {
    const double beta = w[1] / w[3], gamma = w[2] / w[3];
    const double alpha = 1.0 - beta - gamma;
    const PtVec3 A = pt_v3(v[0], v[1], v[2]), B = pt_v3(v[3], v[4], v[5]), C = pt_v3(v[6], v[7], v[8]);
    *p = (A * alpha + B * beta) + C * gamma;
    if (vn) *n = (pt_v3(vn[0], vn[1], vn[2]) * alpha + pt_v3(vn[3], vn[4], vn[5]) * beta) + pt_v3(vn[6], vn[7], vn[8]) * gamma;
    else *n = pt_cross(B - A, C - A);
}

// Step 10: fwd = the node's 12 doubles, nrm = its 9.
PT_HD void pt_chart_world(const double* fwd, const double* nrm, uint32_t flags, PtVec3 p, PtVec3 n, PtVec3* P, PtVec3* N) {
    *P = pt_xform_point(fwd, p);
    const PtVec3 Nw = pt_normalized(pt_xform_dir(nrm, 3, n));
    *N = (flags & PT_CHART_FLAG_FLIP_NORMAL) ? -Nw : Nw;
}

// NOT part of the contract: the texels [x0, x1] x [y0, y1] a triangle's predicate is evaluated on - an optimisation that must hold every texel step 7 accepts.
// A computed edge value has the sign of the exact cross product of two vectors whose components each carry one relative rounding (2^-53), or is zero where
// the two rounded products tie; with coordinates of at most 2^24 an accepted p therefore lies within 2^-25 of each of the three exact half planes. Beyond a
// corner of angle theta those strips overlap for 2^-24 / theta, so for a triangle that is not a sliver the corners' bounding box grown by one texel holds every
// accepted centre. A sliver - |area2| below 2^-20 of its box's larger side squared: theta may be under 2^-21 - is evaluated on the whole map. False: empty.
PT_HD bool pt_chart_box(const double st[6], uint32_t W, uint32_t H, int32_t* x0, int32_t* y0, int32_t* x1, int32_t* y1) {
    const double s_lo = fmin(st[0], fmin(st[2], st[4])), s_hi = fmax(st[0], fmax(st[2], st[4]));
    const double t_lo = fmin(st[1], fmin(st[3], st[5])), t_hi = fmax(st[1], fmax(st[3], st[5]));
    const double ext = fmax(s_hi - s_lo, t_hi - t_lo);
    const double area2 = pt_chart_edge(st[0], st[1], st[2], st[3], st[4], st[5]);
    if (fabs(area2) < (ext * ext) * (1.0 / 1048576.0)) {
        *x0 = 0; *y0 = 0; *x1 = (int32_t)W - 1; *y1 = (int32_t)H - 1;
        return true;
    }
    // (the corners are at most 2^24 in magnitude: the floors fit an int32 with room for the margin)
    const int32_t ax = (int32_t)floor(s_lo) - 1, bx = (int32_t)floor(s_hi) + 1, ay = (int32_t)floor(t_lo) - 1, by = (int32_t)floor(t_hi) + 1;
    *x0 = ax < 0 ? 0 : ax; *y0 = ay < 0 ? 0 : ay;
    *x1 = bx > (int32_t)W - 1 ? (int32_t)W - 1 : bx; *y1 = by > (int32_t)H - 1 ? (int32_t)H - 1 : by;
    return *x0 <= *x1 && *y0 <= *y1;
}

// ---- What pt_api.hip hands pt_chart.hip's three kernels (seed, own, resolve). Every pointer is device memory.
struct PtChartArgs {
    uint32_t width, height, flags, n_tris;
    const double* uv;      // n_tris x 6
    const double* tri_v;   // the mesh's first record
    const double* tri_n;   // likewise, or null: the node shades flat
    const double* fwd;     // the node's 12 doubles
    const double* nrm;     // the node's 9
    uint32_t* owner;       // width x height words, the context's
    double* position;      // the outputs, each optional
    double* normal;
    int32_t* tri;
    uint8_t* covered;
};
#if defined(__HIPCC__)
// which: bit 0 seed + own, bit 1 resolve (profiles/chart/measure.py times them apart through pt_test_chart_phases; a pass queues both)
hipError_t pt_chart_launch(const PtChartArgs& a, int which, hipStream_t stream);
#endif
