// Part of pt_trace.h, which includes it after its own macros (PT_NO_HIT, PT_BLOCK, the PT_DIAG / PT_CYCLES counters): the hit record, the per-lane
// traversal stacks, the f32 slab tests with their error bounds and the walks in which every lane keeps its own node and stack (pt_trace_flat*, PtKdWalker).
#pragma once

struct PtHit {
    double t;       // ray parameter of the best hit so far; doubles as the exclusive range end
    uint32_t node;  // flat node index, PT_NO_HIT when nothing was hit
    uint32_t sub;   // analytic: part tag; mesh / triangle: global triangle index
};

// Per-lane traversal stack: word i of the lane at base[i * PT_BLOCK] (a column of the block's LDS area: a wave's
// pushes and pops hit 64 different banks). PtStack is LDS only (pt_cast_kernel); PtStackSpill keeps the first `cap`
// entries in LDS and the rest - only reached by unusually deep excursions - in HBM, so that the LDS part can be
// sized for the occupancy instead of for the worst case of the deepest tree.
struct PtStack {
    uint32_t* base;
    int cap;
    unsigned int* overflow;  // device word set to 1 when a lane runs out of stack (PT_ERR_TRAVERSAL), in every build
};
struct PtStackSpill {
    uint32_t* base;
    int cap;                 // entries in LDS
    int total;               // entries in all
    uint32_t* gbase;         // entry cap + i of the lane at gbase[i * gstride]
    uint32_t gstride;
    unsigned int* overflow;
};
PT_HD int pt_stack_total(const PtStack& s) { return s.cap; }
PT_HD int pt_stack_total(const PtStackSpill& s) { return s.total; }
// Never expected (pt_scene_upload sizes the stack for the deepest walk); recorded unconditionally so that a render
// whose results would be wrong cannot return PT_OK.
template <class Stack>
PT_HD void pt_stack_overflow(const Stack& s) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (s.overflow) atomicOr(s.overflow, 1u);
#else
    (void)s;
#endif
}

PT_HD void pt_push(const PtStack& s, int& sp, uint32_t v) { s.base[sp * PT_BLOCK] = v; sp++; }
PT_HD uint32_t pt_pop(const PtStack& s, int& sp) { sp--; return s.base[sp * PT_BLOCK]; }
// The HBM part is behind a WAVE-UNIFORM branch (one ballot, one scalar branch): written as a per-lane select the compiler
// turned every pop into a flat load of a computed LDS-or-global address plus eight masked-off address instructions.
PT_HD bool pt_any_lane_beyond(int sp, int cap) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(sp >= cap) != 0ull;
#else
    return sp >= cap;
#endif
}
PT_HD void pt_push(const PtStackSpill& s, int& sp, uint32_t v) {
    if (!pt_any_lane_beyond(sp, s.cap)) s.base[sp * PT_BLOCK] = v;
    else if (sp < s.cap) s.base[sp * PT_BLOCK] = v;
    else s.gbase[(size_t)(sp - s.cap) * s.gstride] = v;
    sp++;
}
PT_HD uint32_t pt_pop(const PtStackSpill& s, int& sp) {
    sp--;
    if (!pt_any_lane_beyond(sp, s.cap)) return s.base[sp * PT_BLOCK];
    if (sp < s.cap) return s.base[sp * PT_BLOCK];
    return s.gbase[(size_t)(sp - s.cap) * s.gstride];
}
template <class Stack>
PT_HD void pt_push_f64(const Stack& s, int& sp, double v) {
    union { double d; uint32_t u[2]; } c; c.d = v;
    pt_push(s, sp, c.u[0]); pt_push(s, sp, c.u[1]);
}
template <class Stack>
PT_HD double pt_pop_f64(const Stack& s, int& sp) {
    union { double d; uint32_t u[2]; } c;
    c.u[1] = pt_pop(s, sp); c.u[0] = pt_pop(s, sp);
    return c.d;
}

// Single-precision ray for the tree walk. The slab test evaluates (plane - o) / d as
// fma(plane, inv, -o * inv) with the per-ray constants rounded so that every error makes the overlap
// LONGER: inv = fl32(1 / d); the lower planes use n0 = -(o_hi * inv), the upper planes n1 = -(o_lo * inv)
// (o_hi >= o >= o_lo bound the f64 origin in f32), each then pushed by 2^-22 relative in the direction
// that moves a near plane nearer and a far plane farther (which plane is near depends on the sign of
// inv). An axis the ray is parallel to (|inv| > 1e18, which also keeps every product below FLT_MAX
// for the |coordinates| <= 1e18 that pt_scene_upload guarantees for boxes) is switched off:
// inv = 0, n0 = -inf, n1 = +inf give the interval (-inf, +inf).
struct PtRay32 {
    float ix, iy, iz, n0x, n0y, n0z, n1x, n1y, n1z;
};
PT_HD void pt_ray32_axis(double o, double d, float* inv, float* n0, float* n1) {
    float x = (float)o;
    const float e = 2.4e-7f;  // > 2^-23: covers the rounding of the conversion and of the bound itself
    float ex = fabsf(x) * e + 1e-37f;
    float oh = x + ex, ol = x - ex;
    float i = (float)(1.0 / d);
    if (!(fabsf(i) <= 1e18f)) {  // parallel (or NaN): no constraint from this axis
        *inv = 0.0f; *n0 = -INFINITY; *n1 = INFINITY;
        return;
    }
    float c0 = oh * i, c1 = ol * i;
    float w0 = fabsf(c0) * 4.8e-7f + 1e-37f, w1 = fabsf(c1) * 4.8e-7f + 1e-37f;
    // i > 0: the lower plane is the near one (make it nearer: larger c0), the upper plane the far one (smaller c1); i < 0: the other way round
    c0 = i > 0.0f ? c0 + w0 : c0 - w0;
    c1 = i > 0.0f ? c1 - w1 : c1 + w1;
    *inv = i; *n0 = -c0; *n1 = -c1;
}
PT_HD PtRay32 pt_ray32(const PtRay& r) {
    PtRay32 q;
    pt_ray32_axis(r.o.x, r.d.x, &q.ix, &q.n0x, &q.n1x);
    pt_ray32_axis(r.o.y, r.d.y, &q.iy, &q.n0y, &q.n1y);
    pt_ray32_axis(r.o.z, r.d.z, &q.iz, &q.n0z, &q.n1z);
    return q;
}

// ---- The same idea with the margins folded into the per-ray constants (round 3; the derivation is with pt_slab_pk2 below): per axis
// a pair (i, c) for a box's LOWER plane and one for its UPPER plane, chosen by the direction's sign so that min / max of the two
// fmas are conservative entering / leaving parameters without any widening afterwards.
typedef float pt_f32x2 __attribute__((ext_vector_type(2)));
struct PtRayPk {
    pt_f32x2 a[3], b[3];  // per axis (i, c) for the children's lower planes / upper planes
};
PT_HD float pt_rcp_f32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
// The constants of one axis, all in f32 (the f64 origin is converted once; -DPT_RAYPK_F64 restores the body that multiplied it in f64).
// With u = 2^-24 (half an ulp), T = (P - o) / d the exact parameter of a plane P (an f32, |P| <= 1e18), and every subnormal result
// allowed to be rounded OR flushed (absolute error <= 2^-126 either way; host and device differ there):
//     i0 = rcp((float)d)             = (1 / d)(1 + e),  |e| < 2^-22.4     (the conversion u, v_rcp_f32 one ulp = 2u; the host's division u).
//                                      Kept only for |i0| <= 1e18, i.e. |d| >= 1e-18: (float)d is normal.
//     lo = fma(|i0|, -2^-21, i0),  hi = fma(|i0|, 2^-21, i0)     one rounding each: lo = i0 -+ |i0| 2^-21 (1 + u'), so for d > 0
//                                      lo <= (1 / d)(1 + 2^-22.4)(1 - 2^-21)(1 + u) < (1 / d)(1 - 2^-22.1) and hi > (1 / d)(1 + 2^-22.1); for d < 0 the
//                                      same with the magnitudes exchanged: lo is i_f, hi is i_n. lo goes with the LOWER planes (A), hi with
//                                      the UPPER ones (B) whatever the sign - what the selects of the f64 body worked out.
//     of = (float)o                  = o (1 + d1) + h1,  |d1| <= u, |h1| <= 2^-126
//     w  = fma(|fl(of i0)|, 2.4e-7, 2e-20)    >= (|o i0| (1 - u)^2 4.02u + 2e-20 - 2^-126 (|i0| + 1) 2.4e-7)(1 - u)
//     c_n = fma(-of, i_n, -w),  c_f = fma(-of, i_f, +w)     ONE rounding each (the product is not rounded on its own), so
//         c_n <= -o i_n + |o i_n| u + 2^-126 |i_n|          (what converting o cost)
//                      + (|o i_n| (1 + u) + 2^-126 |i_n| + w) u + 2^-126        (the fma's rounding)   - w
//             <= -o i_n + |o i_n| (2u + u^2) + 2^-126 (|i_n| + 1)(1 + u) - w (1 - u)   <=   -o i_n
//       because |i_n| <= |i0| <= |i_f| <= |i0| (1 + 2^-21 + 2u) makes the relative part of w at least 4u |o i_n| (1 - 2^-20) - against 2u + u^2
//       needed, for i_f as well - and its constant part 2e-20 (1 - u) - 3e-45 > 1.18e-20 (1 + 3u) >= 2^-126 (1e18 (1 + 2^-20) + 1)(1 + u). c_f >= -o i_f
//       likewise. A subnormal product or sum (either factor tiny) is inside the same constant.
// Entering: fma(P, i_n, c_n) is at most (P - o) i_n before its rounding, which has the sign of T and for T > 0 is at most T (1 - 2^-22.1): the
// rounding (1 + u) cannot lift it above T, and below 2^-126 the constant part of w (at least 0.8e-20 of it is left over) keeps it negative; for
// T <= 0 it stays <= 0 (clamped to 0 or t0 anyway). Leaving: fma(P, i_f, c_f) >= T (1 + 2^-22.1)(1 - u) >= T for T >= 0, by the same argument.
// A switched-off axis takes i0 = +0 and w = +inf through the same expressions: lo = hi = +0, c = fma(-of, 0, -+inf) = -+inf - A = (0, -inf), B = (0, +inf), as
// the f64 body's early return gives them - for a finite (float)o. Where it overflows (|o| >= FLT_MAX) the product is inf x 0 and both c are NaN, which v_max / v_min
// drop as well: the axis is still off, by another route than before.
// All of this for finite o with |o i0| below FLT_MAX; beyond it c_n / c_f become infinities or NaNs of the harmless kind, as they did with the f64
// product (an entering -inf, a leaving +inf; v_max / v_min drop a NaN operand).
// returns 0: axis switched off, 1: positive direction, 2: negative direction
PT_HD int pt_raypk_axis_f32(double o, double d, pt_f32x2* a, pt_f32x2* b) {
    const float r = pt_rcp_f32((float)d);
    const bool on = fabsf(r) <= 1e18f;  // (false for a NaN as well)
    const float i0 = on ? r : 0.0f;
    const float of = (float)o;
    const float k = 4.76837158203125e-7f;  // 2^-21
    const float lo = __builtin_fmaf(fabsf(i0), -k, i0), hi = __builtin_fmaf(fabsf(i0), k, i0);
    const float w = __builtin_fmaf(fabsf(of * i0), 2.4e-7f, 2e-20f);
    const float sw = __builtin_copysignf(on ? w : INFINITY, i0);  // d > 0: A enters (c_n = .. - w), B leaves (c_f = .. + w); d < 0: the other way round
    a->x = lo; a->y = __builtin_fmaf(-of, lo, -sw);
    b->x = hi; b->y = __builtin_fmaf(-of, hi, sw);
    return on ? (r < 0.0f ? 2 : 1) : 0;
}
// the constants as they were computed before, the products with the origin in f64 (derivation: the same with the conversion's u and the margin's own
// rounding in place of the two terms above, 1e-37 for the one subnormal result): -DPT_RAYPK_F64 for an A/B, and what pt_test_raypk compares with
PT_HD int pt_raypk_axis_f64(double o, double d, pt_f32x2* a, pt_f32x2* b) {
    const float i0 = pt_rcp_f32((float)d);
    if (!(fabsf(i0) <= 1e18f)) {
        a->x = 0.0f; a->y = -INFINITY; b->x = 0.0f; b->y = INFINITY;
        return 0;
    }
    const float k = 4.76837158203125e-7f;  // 2^-21
    const float in = i0 - i0 * k, fi = i0 + i0 * k;
    float cn = (float)(-(o * (double)in)), cf = (float)(-(o * (double)fi));
    cn = cn - (fabsf(cn) * 2.4e-7f + 1e-37f);
    cf = cf + (fabsf(cf) * 2.4e-7f + 1e-37f);
    const bool neg = i0 < 0.0f;  // entering through the upper plane
    a->x = neg ? fi : in; a->y = neg ? cf : cn;
    b->x = neg ? in : fi; b->y = neg ? cn : cf;
    return neg ? 2 : 1;
}
PT_HD int pt_raypk_axis(double o, double d, pt_f32x2* a, pt_f32x2* b) {
#ifdef PT_RAYPK_F64
    return pt_raypk_axis_f64(o, d, a, b);
#else
    return pt_raypk_axis_f32(o, d, a, b);
#endif
}
PT_HD PtRayPk pt_raypk(const PtRay& r) {  // without the wavefront's view: for walks that always take the per-lane form
    PtRayPk q;
    pt_raypk_axis(r.o.x, r.d.x, &q.a[0], &q.b[0]);
    pt_raypk_axis(r.o.y, r.d.y, &q.a[1], &q.b[1]);
    pt_raypk_axis(r.o.z, r.d.z, &q.a[2], &q.b[2]);
    return q;
}
// The per-lane form of the slab test with those constants, against a segment [tmin, tmax] of the ray (both already rounded outward
// by the caller): the conservative culls of the k-d walks. 6 fmas + 6 min / max + 4 + 1 compare.
PT_HD bool pt_slab_seg_pk(const float* lo, const float* hi, const PtRayPk& q, float tmin, float tmax) {
    const float ax = __builtin_fmaf(lo[0], q.a[0].x, q.a[0].y), bx = __builtin_fmaf(hi[0], q.b[0].x, q.b[0].y);
    const float ay = __builtin_fmaf(lo[1], q.a[1].x, q.a[1].y), by = __builtin_fmaf(hi[1], q.b[1].x, q.b[1].y);
    const float az = __builtin_fmaf(lo[2], q.a[2].x, q.a[2].y), bz = __builtin_fmaf(hi[2], q.b[2].x, q.b[2].y);
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax));
    return !(tn > tf);
}

// Slab test of one child box against [0, tmax] in f32. Conservative by construction (see PtRay32);
// the final interval is widened by 2^-20 relative (fma + reciprocal roundings are < 2^-22), NaNs
// cannot arise from finite boxes, and the comparison is written so that an unordered result accepts
// the box anyway.
PT_HD bool pt_slab32(const float* lo, const float* hi, const PtRay32& q, float tmax, float* tnear) {
    float x0 = __builtin_fmaf(lo[0], q.ix, q.n0x), x1 = __builtin_fmaf(hi[0], q.ix, q.n1x);
    float y0 = __builtin_fmaf(lo[1], q.iy, q.n0y), y1 = __builtin_fmaf(hi[1], q.iy, q.n1y);
    float z0 = __builtin_fmaf(lo[2], q.iz, q.n0z), z1 = __builtin_fmaf(hi[2], q.iz, q.n1z);
    float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    const float w = 9.6e-7f;
    tn = fmaxf(__builtin_fmaf(fabsf(tn), -w, tn), 0.0f);
    tf = fminf(__builtin_fmaf(fabsf(tf), w, tf), tmax);
    *tnear = tn;
    return !(tn > tf);
}

// The four child boxes of a PtBvh4Node against [0, tmax]: pt_slab32 four times over the node's [axis][child] arrays.
// tn[k] = entry distance of child k, +inf where the box is missed or the slot is unused.
PT_HD void pt_slab32_x4(const PtBvh4Node& n, const PtRay32& q, float tmax, float tn[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float x0 = __builtin_fmaf(n.lo[0][k], q.ix, q.n0x), x1 = __builtin_fmaf(n.hi[0][k], q.ix, q.n1x);
        float y0 = __builtin_fmaf(n.lo[1][k], q.iy, q.n0y), y1 = __builtin_fmaf(n.hi[1][k], q.iy, q.n1y);
        float z0 = __builtin_fmaf(n.lo[2][k], q.iz, q.n0z), z1 = __builtin_fmaf(n.hi[2][k], q.iz, q.n1z);
        float a = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
        float f = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
        const float w = 9.6e-7f;
        a = fmaxf(__builtin_fmaf(fabsf(a), -w, a), 0.0f);
        f = fminf(__builtin_fmaf(fabsf(f), w, f), tmax);
        tn[k] = (!(a > f) && n.child[k] != PT_REF_EMPTY) ? a : INFINITY;
    }
}
// Compare-exchange of (distance, reference) pairs: after the five of pt_sort4 the hit children are in order of entry
// distance, misses (+inf) last. Order only decides how soon `tmax` shrinks, never a result.
#define PT_CSWAP(i, j) do { const bool sw_ = t[j] < t[i]; const float tt_ = sw_ ? t[j] : t[i]; t[j] = sw_ ? t[i] : t[j]; t[i] = tt_; \
                            const uint32_t cc_ = sw_ ? c[j] : c[i]; c[j] = sw_ ? c[i] : c[j]; c[i] = cc_; } while (0)
PT_HD void pt_sort4(float t[4], uint32_t c[4]) {
    PT_CSWAP(0, 1); PT_CSWAP(2, 3); PT_CSWAP(0, 2); PT_CSWAP(1, 3); PT_CSWAP(1, 2);
}

// Generic walk of the build's two-child tree, "while-while": every lane first descends through inner
// nodes until it holds a leaf (or has nothing left), and only then do the lanes test their leaves
// together — the leaf work (f64 primitive tests) is the expensive part and should run with as many
// lanes active as possible. leaf(first, count, sp) tests the items and returns true to stop the walk
// (any-hit). `tmax` is re-read after every leaf so shrinking it culls.
template <bool STATS, class Stack, class Leaf>
PT_HD bool pt_bvh_walk(const PtBvh4Node* nodes, uint32_t root, const PtRay& r, const double& tmax,
                       const Stack& stk, int sp0, Leaf&& leaf, PtCounters* cnt) {
    if (root == PT_REF_EMPTY) return false;
    int sp = sp0;
    const PtRay32 q = pt_ray32(r);
    uint32_t cur = root;
    for (;;) {
        while (!(cur & PT_REF_LEAF)) {
            const PtBvh4Node& n = nodes[cur];
            if (STATS) cnt->n_inner++;
            PT_WAVE_COUNT(4);
            // tmax rounded up: (float) rounds to nearest, one more relative step covers it (inf stays inf)
            float tm = (float)tmax; tm = tm + fabsf(tm) * 2.4e-7f;
            float t[4];
            uint32_t c[4] = {n.child[0], n.child[1], n.child[2], n.child[3]};
            pt_slab32_x4(n, q, tm, t);
            pt_sort4(t, c);
            if (!(t[0] < INFINITY)) {
                if (sp == sp0) return false;
                cur = pt_pop(stk, sp);
                continue;
            }
            const int hits = (t[1] < INFINITY) + (t[2] < INFINITY) + (t[3] < INFINITY);
            if (sp + hits > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; return false; }
            if (t[3] < INFINITY) pt_push(stk, sp, c[3]);
            if (t[2] < INFINITY) pt_push(stk, sp, c[2]);
            if (t[1] < INFINITY) pt_push(stk, sp, c[1]);
            cur = c[0];
        }
        if (STATS) cnt->n_leaf++;
        PT_WAVE_COUNT(5);
        if (leaf((cur & ~PT_REF_LEAF) >> 3, (cur & 7u) + 1u, sp)) return true;
        if (sp == sp0) return false;
        cur = pt_pop(stk, sp);
    }
}

// The same walk over the two-child form (mesh-free scenes: see PtBvhWalker::step).
template <bool STATS, class Stack, class Leaf>
PT_HD bool pt_bvh2_walk(const PtBvhNode* nodes, uint32_t root, const PtRay& r, const double& tmax,
                       const Stack& stk, int sp0, Leaf&& leaf, PtCounters* cnt) {
    if (root == PT_REF_EMPTY) return false;
    int sp = sp0;
    const PtRay32 q = pt_ray32(r);
    uint32_t cur = root;
    for (;;) {
        while (!(cur & PT_REF_LEAF)) {
            const PtBvhNode& n = nodes[cur];
            if (STATS) cnt->n_inner++;
            PT_WAVE_COUNT(4);
            // tmax rounded up: (float) rounds to nearest, one more relative step covers it (inf stays inf)
            float tm = (float)tmax; tm = tm + fabsf(tm) * 2.4e-7f;
            float t0, t1, lo0[3], hi0[3], lo1[3], hi1[3];
            pt_node_get_box(n, 0, lo0, hi0); pt_node_get_box(n, 1, lo1, hi1);
            bool h0 = pt_slab32(lo0, hi0, q, tm, &t0);
            bool h1 = pt_slab32(lo1, hi1, q, tm, &t1);
            uint32_t c0 = n.child0, c1 = n.child1;
            if (h0 && h1) {
                bool swap = t1 < t0;
                if (sp + 1 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; return false; }
                pt_push(stk, sp, swap ? c0 : c1);
                cur = swap ? c1 : c0;
            } else if (h0) {
                cur = c0;
            } else if (h1) {
                cur = c1;
            } else {
                if (sp == sp0) return false;
                cur = pt_pop(stk, sp);
            }
        }
        if (STATS) cnt->n_leaf++;
        PT_WAVE_COUNT(5);
        { PT_CYC_BEGIN(); const bool stop_ = leaf((cur & ~PT_REF_LEAF) >> 3, (cur & 7u) + 1u, sp); PT_CYC_END(5); if (stop_) return true; }
        if (sp == sp0) return false;
        cur = pt_pop(stk, sp);
    }
}

// Exclusive range end for a candidate: t == best.t is admitted only when the candidate comes
// before the current winner in flat order (ray.rs:87-99: the first of equal hits wins).
PT_HD double pt_cand_end(const PtHit& best, uint32_t node, uint32_t sub) {
    bool before = best.node != PT_NO_HIT && (node < best.node || (node == best.node && sub < best.sub));
    return before ? pt_next_up(best.t) : best.t;
}

// The same for the hierarchical traversal: between different nodes the one that comes first depth-first wins
// (scene.rs:95-117: own geometry, then the children in order, each a half-open shrinking range).
template <bool HIER>
PT_HD double pt_cand_end_in(const PtSceneView& sc, const PtHit& best, uint32_t node, uint32_t sub) {
    if (!HIER) return pt_cand_end(best, node, sub);
    bool before = best.node != PT_NO_HIT && (node == best.node ? sub < best.sub : sc.dfs_rank[node] < sc.dfs_rank[best.node]);
    return before ? pt_next_up(best.t) : best.t;
}

// World-space ray -> the node's model space. FLAT: the flattened node's composed inverse (flat_scene.rs:74).
// HIER: one SceneNode at a time down the path, each with its own inverse (scene.rs:82) - the same transform in
// exact arithmetic, different roundings.
template <bool HIER>
PT_HD PtRay pt_node_local_ray(const PtSceneView& sc, uint32_t node, const PtRay& ray) {
    if (!HIER) return pt_ray_to_local(sc.inv + 12 * (size_t)node, ray);
    PtRay r = ray;
    const uint32_t* rec = sc.hier_rec + 8 * (size_t)node;  // the node's path in one 32-byte line (pt_api.hip) instead of chain_off -> chain
    const uint32_t len = rec[0] & 255u;
    if (len == 255u) {  // more than seven levels
        for (uint32_t k = sc.chain_off[node]; k < sc.chain_off[node + 1]; k++) r = pt_ray_to_local(sc.g_inv + 12 * (size_t)sc.chain[k], r);
        return r;
    }
    for (uint32_t k = 0; k < len; k++) r = pt_ray_to_local(sc.g_inv + 12 * (size_t)rec[1 + k], r);
    return r;
}

PT_HD double pt_axis(PtVec3 v, int axis) { return axis == 0 ? v.x : (axis == 1 ? v.y : v.z); }

// KDMesh::ray_hit (kdtree/kdmesh.rs:62-74): box test on the tree's root bounds, then the mesh's OWN
// k-d tree of triangles walked exactly like the scene tree (node.rs:33-51 + :66-203): front to back,
// range clipped at straddled planes, the first leaf with a hit wins, and — quirk Q3 — the segment used
// to classify sides ends at start + extent (squared diagonal), so hits farther away than that can be
// missed. Reproduced because results differ from Mesh whenever the quirk bites.
template <bool STATS, class Stack>
PT_HD bool pt_kdmesh_hit(const PtSceneView& sc, const PtMeshInfo& m, const PtRay& local, double start, double end, const Stack& stk,
                         int sp0, double* t_out, uint32_t* tri_out, PtCounters* cnt) {
    if (STATS) cnt->n_bbox++;
    if (!pt_bbox_test_hit(m.kd_bbox_inv, local, start, end)) return false;
    int sp = sp0;
    int32_t cur = m.kd_root;
    const double extent = m.kd_extent;
    const double end0 = end;  // a pending far side's range end = the start of the entry below it, or end0
    const PtRayPk q = pt_raypk(local);
    for (;;) {
        const PtKdNode n = sc.mkd[cur];
        // conservative culls as in pt_trace_kd: a subtree / a triangle whose box the segment [start, end) does not reach reports no hit
        float seg0 = (float)start, seg1 = (float)end;
        seg0 = seg0 - fabsf(seg0) * 2.4e-7f; seg1 = seg1 + fabsf(seg1) * 2.4e-7f;
        if (sc.mkd_box && !pt_slab_seg_pk(n.box, n.box + 3, q, seg0, seg1)) {
            if (STATS) cnt->kd_culled++;
        } else if (n.axis < 0) {  // leaf: [T]::ray_hit (ray.rs:50-63) over the leaf's triangles, in order, strict shrinking end
            if (STATS) cnt->n_leaf++;
            bool found = false;
            double e = end;
            for (int32_t i = 0; i < n.count; i++) {
                uint32_t tri = sc.mkd_items[n.first + i];
                if (sc.mkd_item_box) {
                    const float* ib = sc.mkd_item_box + 6 * (size_t)(n.first + i);
                    if (!pt_slab_seg_pk(ib, ib + 3, q, seg0, seg1)) continue;
                }
                double tt, beta, gamma;
                if (STATS) cnt->n_tri++;
                if (pt_triangle_hit(sc.tri_v + 9 * (size_t)tri, local, start, e, &tt, &beta, &gamma)) { e = tt; *t_out = tt; *tri_out = tri; found = true; }
            }
            if (found) return true;
        } else {
            if (STATS) cnt->n_inner++;
            double t_max = start + extent;
            if (!pt_in_range(start, end, t_max)) t_max = end - PT_EPSILON;
            double t_min = start + PT_EPSILON;
            double o = pt_axis(local.o, n.axis), d = pt_axis(local.d, n.axis);
            bool s = ((o + d * t_min) - n.plane) >= 0.0;
            bool e = ((o + d * t_max) - n.plane) >= 0.0;
            if (s == e) { cur = s ? n.front : n.back; continue; }
            double plane_t = (n.plane - o) / d;
            if (pt_in_range(start, end, plane_t)) {
                if (sp + 3 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; return false; }
                pt_push(stk, sp, (uint32_t)(s ? n.back : n.front));  // pending far side: (node, start = plane_t)
                pt_push_f64(stk, sp, plane_t);
                cur = s ? n.front : n.back;
                end = plane_t;
                continue;
            }
            if (STATS) cnt->kd_plane_miss++;  // node.rs:146-147 / :177-178 would panic
        }
        if (sp == sp0) return false;
        start = pt_pop_f64(stk, sp);
        cur = (int32_t)pt_pop(stk, sp);
        if (sp == sp0) end = end0;
        else { int peek = sp; end = pt_pop_f64(stk, peek); }
    }
}

// flat_scene.rs:71-99 for one flattened node: transform the ray into model space, dispatch on the
// primitive (primitive.rs:55-62), keep the hit if it beats `best`. Returns true if best changed.
template <bool STATS, bool MESH = true, class Stack = PtStack>
PT_HD bool pt_test_node(const PtSceneView& sc, uint32_t node, const PtRay& ray, double start, PtHit& best, bool any,
                        const Stack& stk, int sp, PtCounters* cnt) {
    const uint32_t* info = sc.info + 4 * (size_t)node;
    uint32_t type = info[0], data = info[1];
    PtRay local = pt_ray_to_local(sc.inv + 12 * (size_t)node, ray);
    if (STATS) cnt->n_analytic++;
    double t;
    uint32_t part = 0;
    bool hit;
    switch (type) {
    case PT_SPHERE: case PT_PLANE: case PT_CUBE: case PT_CYLINDER: case PT_CONE:
        hit = pt_unit_prim_hit(type, local, start, pt_cand_end(best, node, 0), &t, &part);
        break;
    case PT_TRIANGLE: {  // stand-alone triangle, stored after the mesh triangles
        double beta, gamma;
        if (STATS) cnt->n_tri++;
        hit = pt_triangle_hit(sc.tri_v + 9 * (size_t)data, local, start, pt_cand_end(best, node, data), &t, &beta, &gamma);
        part = data;
        break;
    }
    default: {  // PT_MESH / PT_KDMESH: mesh.rs:146-167 (box test, then the nearest triangle)
        if (!MESH) return false;  // PT_MODE_FLAT_NOMESH: the host guarantees there is none
        const PtMeshInfo& m = sc.meshes[data];
        if (type == PT_KDMESH && m.kd_root >= 0) {
            uint32_t tri = 0;
            if (!pt_kdmesh_hit<STATS>(sc, m, local, start, pt_cand_end(best, node, 0), stk, sp, &t, &tri, cnt)) return false;
            best.t = t; best.node = node; best.sub = tri;
            return true;
        }
        if (STATS) cnt->n_bbox++;
        if (!pt_bbox_test_hit(m.bbox_inv, local, start, pt_cand_end(best, node, 0))) return false;
        bool changed = false;
        const double* tri_v = sc.tri_v;
        pt_bvh_walk<STATS>(sc.bvh4, m.blas_root, local, best.t, stk, sp,
            [&](uint32_t first, uint32_t count, int) -> bool {
                for (uint32_t i = 0; i < count; i++) {
                    uint32_t tri = sc.bvh_items[first + i];
                    double tt, beta, gamma;
                    if (STATS) cnt->n_tri++;
                    if (pt_triangle_hit(tri_v + 9 * (size_t)tri, local, start, pt_cand_end(best, node, tri), &tt, &beta, &gamma)) {
                        best.t = tt; best.node = node; best.sub = tri;
                        changed = true;
                        if (any) return true;
                    }
                }
                return false;
            }, cnt);
        return changed;
    }
    }
    if (!hit) return false;
    best.t = t; best.node = node; best.sub = part;
    return true;
}

// FLAT mode for scenes WITHOUT mesh instances: the generic walk with a one-node leaf handler.
// (Measured 4 % faster on big-scene than the two-level loop below with its mesh path compiled out:
// fewer loop-carried registers.)
template <bool STATS, class Stack>
PT_HD bool pt_trace_flat_simple(const PtSceneView& sc, const PtRay& ray, bool any, PtHit& best, const Stack& stk, PtCounters* cnt) {
    best.t = INFINITY; best.node = PT_NO_HIT; best.sub = 0;
    if (sc.n_nodes == 0) return false;
    pt_bvh2_walk<STATS>(sc.bvh, sc.tlas_root, ray, best.t, stk, 0,
        [&](uint32_t first, uint32_t count, int sp) -> bool {
            for (uint32_t i = 0; i < count; i++) {
                uint32_t node = sc.tlas_direct ? first : sc.bvh_items[first + i];
                if (pt_test_node<STATS, false>(sc, node, ray, PT_EPSILON, best, any, stk, sp, cnt) && any) return true;
            }
            return false;
        }, cnt);
    return best.node != PT_NO_HIT;
}

// FLAT mode: nearest hit over [EPSILON, inf) (ray.rs:139-141), or any hit for shadow rays
// (material.rs:174-179 only asks is_none()).
//
// `any` is a per-lane run-time flag, not a template parameter: lanes carrying shadow rays and lanes
// carrying primary / secondary rays walk the tree together in one instruction stream. The scene tree
// and the per-mesh triangle trees are walked by ONE loop: entering a mesh instance pushes a marker,
// switches the lane to the instance's model-space ray (ray.rs:130-135: same t in both spaces) and
// continues in the mesh's tree; popping the marker switches back. Lanes inside a mesh and lanes in
// the scene tree therefore share the inner-node code instead of waiting for each other.
#define PT_REF_MARKER 0xFFFFFFFEu
#define PT_REF_POP 0xFFFFFFFDu     // inside a walk: "take the next pending subtree" (never stored)
// The walk of the build's two-level bounding-volume tree as a resumable machine: begin() takes a ray, every step() is one
// round of the "while-while" loop - down through inner nodes to a leaf, the leaf's candidates, the next pending subtree -
// and returns true once the ray is finished (result in `best`). pt_render_kernel drives it so that a lane whose ray is
// finished can take its NEXT ray while its neighbours are still walking (pt_render_kernel.h); pt_trace_flat() below runs
// it to the end for one ray.
// MESH = false compiles the mesh-instance path out (scenes of analytic primitives and stand-alone
// triangles only): fewer live registers in the hot loop.
template <bool MESH, bool KDMESH = MESH, bool HIER = false>
struct PtBvhWalker {
    PtHit best;
    int sp;
    uint32_t cur;
    PtRay32 q;
    PtRay local;    // model-space ray of the mesh instance being walked
    uint32_t inst;  // flat node index of that instance, PT_NO_HIT while in the scene tree

    PT_HD bool begin(const PtSceneView& sc, const PtRay& ray) {  // false: nothing to walk, the ray is finished (a miss)
        best.t = INFINITY; best.node = PT_NO_HIT; best.sub = 0;
        sp = 0; inst = PT_NO_HIT; cur = sc.tlas_root;
        if (MESH) local = ray;
        if (sc.n_nodes == 0 || sc.tlas_root == PT_REF_EMPTY) return false;
        q = pt_ray32(ray);
        return true;
    }

    template <bool STATS, class Stack>
    PT_HD bool step(const PtSceneView& sc, const PtRay& ray, bool any, const Stack& stk, PtCounters* cnt) {
        // Scenes WITH mesh instances walk the four-child form of the trees: half as many dependent node fetches, which is
        // what a walk through a tree far larger than the caches waits for (big-soup +8 %, mirror +2 %). Mesh-free scenes
        // (their one tree is cache-resident) keep the two-child form: the same instruction count per level pair, and the
        // finer front-to-back order shrinks tmax sooner (big-scene 2.5 % faster than on the four-child form).
        while (MESH && !(cur & PT_REF_LEAF)) {
            const PtBvh4Node& n = sc.bvh4[cur];
            if (STATS) cnt->n_inner++;
            PT_WAVE_COUNT(4);
            float tm = (float)best.t; tm = tm + fabsf(tm) * 2.4e-7f;
            float t[4];
            uint32_t c[4] = {n.child[0], n.child[1], n.child[2], n.child[3]};
            pt_slab32_x4(n, q, tm, t);
            pt_sort4(t, c);
            if (!(t[0] < INFINITY)) {
                cur = PT_REF_EMPTY;  // nothing below: take the next pending subtree
                break;
            }
            const int hits = (t[1] < INFINITY) + (t[2] < INFINITY) + (t[3] < INFINITY);
            if (sp + hits > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; best.node = PT_NO_HIT; return true; }
            if (t[3] < INFINITY) pt_push(stk, sp, c[3]);
            if (t[2] < INFINITY) pt_push(stk, sp, c[2]);
            if (t[1] < INFINITY) pt_push(stk, sp, c[1]);
            cur = c[0];
        }
        while (!MESH && !(cur & PT_REF_LEAF)) {
            const PtBvhNode& n = sc.bvh[cur];
            if (STATS) cnt->n_inner++;
            PT_WAVE_COUNT(4);
            float tm = (float)best.t; tm = tm + fabsf(tm) * 2.4e-7f;
            float t0, t1, lo0[3], hi0[3], lo1[3], hi1[3];
            pt_node_get_box(n, 0, lo0, hi0); pt_node_get_box(n, 1, lo1, hi1);
            bool h0 = pt_slab32(lo0, hi0, q, tm, &t0);
            bool h1 = pt_slab32(lo1, hi1, q, tm, &t1);
            uint32_t c0 = n.child0, c1 = n.child1;
            if (h0 && h1) {
                bool swap = t1 < t0;
                if (sp + 1 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; best.node = PT_NO_HIT; return true; }
                pt_push(stk, sp, swap ? c0 : c1);
                cur = swap ? c1 : c0;
            } else if (h0) {
                cur = c0;
            } else if (h1) {
                cur = c1;
            } else {
                cur = PT_REF_EMPTY;  // nothing below: take the next pending subtree
                break;
            }
        }
        if (cur != PT_REF_EMPTY && cur != PT_REF_MARKER) {
            if (STATS) cnt->n_leaf++;
            PT_WAVE_COUNT(5);
            const uint32_t first = (cur & ~PT_REF_LEAF) >> 3, count = (cur & 7u) + 1u;
            bool entered = false;
            for (uint32_t i = 0; i < count && !entered; i++) {
                uint32_t item = ((!MESH || inst == PT_NO_HIT) && sc.tlas_direct) ? first : sc.bvh_items[first + i];
                if (MESH && inst != PT_NO_HIT) {  // a triangle of the current mesh instance (mesh.rs:157-166, triangle.rs:38-80)
                    double tt, beta, gamma;
                    if (STATS) cnt->n_tri++;
                    if (pt_triangle_hit(sc.tri_v + 9 * (size_t)item, local, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, inst, item), &tt, &beta, &gamma)) {
                        best.t = tt; best.node = inst; best.sub = item;
                        if (any) return true;
                    }
                    continue;
                }
                const uint32_t* info = sc.info + 4 * (size_t)item;
                uint32_t type = info[0], data = info[1];
                PtRay lr = pt_node_local_ray<HIER>(sc, item, ray);  // flat_scene.rs:74
                if (STATS) cnt->n_analytic++;
                if (MESH && KDMESH && type == PT_KDMESH && sc.meshes[data].kd_root >= 0) {  // the reference's own triangle tree (quirk Q3)
                    double t; uint32_t tri = 0;
                    if (pt_kdmesh_hit<STATS>(sc, sc.meshes[data], lr, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, item, 0), stk, sp, &t, &tri, cnt)) {
                        best.t = t; best.node = item; best.sub = tri;
                        if (any) return true;
                    }
                } else if (MESH && (type == PT_MESH || type == PT_KDMESH)) {  // mesh.rs:146-155: box test, then the triangles
                    const PtMeshInfo& m = sc.meshes[data];
                    if (STATS) cnt->n_bbox++;
                    if (m.blas_root == PT_REF_EMPTY || !pt_bbox_test_hit(m.bbox_inv, lr, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, item, 0))) continue;
                    if (sp + 2 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; best.node = PT_NO_HIT; return true; }
                    // remaining items of this leaf (scene leaves hold one node unless PORTRAYER_TLAS_LEAF > 1)
                    if (i + 1 < count) pt_push(stk, sp, PT_REF_LEAF | ((first + i + 1) << 3) | (count - i - 2));
                    pt_push(stk, sp, PT_REF_MARKER);
                    local = lr; q = pt_ray32(lr); inst = item;
                    cur = m.blas_root;
                    entered = true;
                } else {
                    double t; uint32_t part = 0; bool hit;
                    if (type == PT_TRIANGLE) {
                        double beta, gamma;
                        if (STATS) cnt->n_tri++;
                        hit = pt_triangle_hit(sc.tri_v + 9 * (size_t)data, lr, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, item, data), &t, &beta, &gamma);
                        part = data;
                    } else {
                        hit = pt_unit_prim_hit(type, lr, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, item, 0), &t, &part);
                    }
                    if (hit) {
                        best.t = t; best.node = item; best.sub = part;
                        if (any) return true;
                    }
                }
            }
            if (entered) return false;
        }
        // next pending subtree
        for (;;) {
            if (sp == 0) return true;
            cur = pt_pop(stk, sp);
            if (!MESH || cur != PT_REF_MARKER) break;
            q = pt_ray32(ray); inst = PT_NO_HIT;  // leaving the mesh instance: back to the world-space ray
        }
        return false;
    }
};

// FLAT mode: nearest hit over [EPSILON, inf) (ray.rs:139-141), or any hit for shadow rays (material.rs:174-179 only
// asks is_none()), for ONE ray.
template <bool STATS, bool MESH, bool KDMESH = MESH, bool HIER = false, class Stack = PtStack>
PT_HD bool pt_trace_flat(const PtSceneView& sc, const PtRay& ray, bool any, PtHit& best, const Stack& stk, PtCounters* cnt) {
    PtBvhWalker<MESH, KDMESH, HIER> w;
    if (w.begin(sc, ray))
        while (!w.template step<STATS>(sc, ray, any, stk, cnt)) {}
    best = w.best;
    return best.node != PT_NO_HIT;
}

// The reference's k-d walk (kdtree/node.rs:112-202) as a resumable machine like PtBvhWalker. A pending far side is
// (node, start) = 3 words: its range end is the start of the entry below it on the stack (or +inf), because the current
// `end` always equals the plane parameter of the innermost straddled split whose near side is being walked.
//
// MESH = false (scenes of analytic primitives): "while-while" - a step works through splits, culls and pops until the
// lane holds a LEAF, then the lanes run the leaf code (the f32 boxes of the leaf's references and the f64 primitive
// tests, an order of magnitude more instructions than a split step) together.
// MESH = true: a step is ONE node, split or leaf - with mesh instances a leaf can hold a whole mesh-tree walk, and the
// while-while form made every lane wait for it (mirror KD 7.1 -> 6.7 Gray/s, profiles/r02/notes.md).
template <bool MESH>
struct PtKdWalker {
    PtHit best;
    double start, end;
    int sp;
    int32_t cur;
    PtRayPk q;
    static constexpr int32_t NONE = -1;

    PT_HD bool begin(const PtSceneView& sc, const PtRay& ray) {
        best.t = INFINITY; best.node = PT_NO_HIT; best.sub = 0;
        start = PT_EPSILON; end = INFINITY;  // ray.rs:140
        sp = 0; cur = 0;
        q = pt_raypk(ray);
        return true;
    }

    template <bool STATS, class Stack>
    PT_HD bool step(const PtSceneView& sc, const PtRay& ray, bool any, const Stack& stk, PtCounters* cnt) {
        const double extent = sc.kd_extent;
        if (MESH) return step_one_node<STATS>(sc, ray, any, stk, cnt, extent);
        return step_to_leaf<STATS>(sc, ray, any, stk, cnt, extent);
    }

    template <bool STATS, class Stack>
    PT_HD bool step_one_node(const PtSceneView& sc, const PtRay& ray, bool any, const Stack& stk, PtCounters* cnt, const double extent) {
        const PtKdNode n = sc.kd[cur];
        // The ray's segment [start, end), rounded outward, against conservative f32 boxes: first the union of
        // everything below this tree node - a subtree the segment does not reach reports no hit, which is all
        // the reference would find out by walking it - then, in a leaf, each referenced node's own box.
        float seg0 = (float)start, seg1 = (float)end;
        seg0 = seg0 - fabsf(seg0) * 2.4e-7f; seg1 = seg1 + fabsf(seg1) * 2.4e-7f;
        if (sc.kd_box && !pt_slab_seg_pk(n.box, n.box + 3, q, seg0, seg1)) {
            if (STATS) cnt->kd_culled++;
        } else if (n.axis < 0) {  // Leaf: ray.rs:87-99 fold over the leaf's nodes, reference order, strict ends
            if (STATS) cnt->n_leaf++;
            bool found = false;
            // The reference's tree puts a node into every leaf its box touches (6.8 references per node on
            // big-scene) and tests all of them. A node whose (padded, outward-rounded) world box the ray's
            // segment [start, end) does not reach cannot report a hit in that range, so it is skipped before
            // the f64 test: same answers, 60 instead of 2 exact tests per ray saved.
            for (int32_t i = 0; i < n.count; i++) {
                const uint32_t item = sc.kd_items[n.first + i];
                if (sc.node_box) {
                    const float* b = sc.node_box + 6 * (size_t)(n.first + i);
                    if (STATS) cnt->n_bbox++;
                    if (!pt_slab_seg_pk(b, b + 3, q, seg0, seg1)) continue;
                }
                PtHit lb; lb.t = end; lb.node = PT_NO_HIT; lb.sub = 0;
                if (pt_test_node<STATS>(sc, item, ray, start, lb, any, stk, sp, cnt)) {
                    best = lb; end = lb.t; found = true;
                    if (any) return true;
                }
            }
            if (found) return true;  // node.rs:153-157: the first side that hits wins
        } else {
            if (STATS) cnt->n_inner++;
            double t_max = start + extent;                                   // node.rs:118
            if (!pt_in_range(start, end, t_max)) t_max = end - PT_EPSILON;   // node.rs:121
            double t_min = start + PT_EPSILON;                               // node.rs:124
            double o = pt_axis(ray.o, n.axis), d = pt_axis(ray.d, n.axis);
            bool s = ((o + d * t_min) - n.plane) >= 0.0;                     // infinite_plane.rs:27-35
            bool e = ((o + d * t_max) - n.plane) >= 0.0;
            if (s == e) { cur = s ? n.front : n.back; return false; }
            double plane_t = (n.plane - o) / d;                              // node.rs:90-109
            if (pt_in_range(start, end, plane_t)) {
                if (sp + 3 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; best.node = PT_NO_HIT; return true; }
                pt_push(stk, sp, (uint32_t)(s ? n.back : n.front));
                pt_push_f64(stk, sp, plane_t);
                cur = s ? n.front : n.back;
                end = plane_t;
                return false;
            }
            // node.rs:146-147 / :177-178: the reference panics here; report a miss for this subtree
            if (STATS) cnt->kd_plane_miss++;
        }
        if (sp == 0) { return true; }
        start = pt_pop_f64(stk, sp);
        cur = (int32_t)pt_pop(stk, sp);
        if (sp == 0) end = INFINITY;
        else { int peek = sp; end = pt_pop_f64(stk, peek); }
        return false;
    }

    template <bool STATS, class Stack>
    PT_HD bool step_to_leaf(const PtSceneView& sc, const PtRay& ray, bool any, const Stack& stk, PtCounters* cnt, const double extent) {
        PtKdNode n;
        float seg0 = 0.0f, seg1 = 0.0f;
        bool finished = false;
        for (;;) {  // until this lane holds a leaf whose bounds its segment reaches
            if (cur == NONE) {  // next pending far side
                if (sp == 0) { finished = true; break; }
                start = pt_pop_f64(stk, sp);
                cur = (int32_t)pt_pop(stk, sp);
                if (sp == 0) end = INFINITY;
                else { int peek = sp; end = pt_pop_f64(stk, peek); }
            }
            n = sc.kd[cur];
            PT_WAVE_COUNT(4);
            // The ray's segment [start, end), rounded outward, against conservative f32 boxes: first the union of
            // everything below this tree node - a subtree the segment does not reach reports no hit, which is all
            // the reference would find out by walking it - then, in a leaf, each referenced node's own box.
            seg0 = (float)start; seg1 = (float)end;
            seg0 = seg0 - fabsf(seg0) * 2.4e-7f; seg1 = seg1 + fabsf(seg1) * 2.4e-7f;
            if (sc.kd_box && !pt_slab_seg_pk(n.box, n.box + 3, q, seg0, seg1)) {
                if (STATS) cnt->kd_culled++;
                cur = NONE;
                continue;
            }
            if (n.axis < 0) break;  // a leaf to test
            if (STATS) cnt->n_inner++;
            double t_max = start + extent;                                   // node.rs:118
            if (!pt_in_range(start, end, t_max)) t_max = end - PT_EPSILON;   // node.rs:121
            double t_min = start + PT_EPSILON;                               // node.rs:124
            double o = pt_axis(ray.o, n.axis), d = pt_axis(ray.d, n.axis);
            bool s = ((o + d * t_min) - n.plane) >= 0.0;                     // infinite_plane.rs:27-35
            bool e = ((o + d * t_max) - n.plane) >= 0.0;
            if (s == e) { cur = s ? n.front : n.back; continue; }
            double plane_t = (n.plane - o) / d;                              // node.rs:90-109
            if (pt_in_range(start, end, plane_t)) {
                if (sp + 3 > pt_stack_total(stk)) { pt_stack_overflow(stk); if (STATS) cnt->stack_overflow++; best.node = PT_NO_HIT; return true; }
                pt_push(stk, sp, (uint32_t)(s ? n.back : n.front));
                pt_push_f64(stk, sp, plane_t);
                cur = s ? n.front : n.back;
                end = plane_t;
                continue;
            }
            // node.rs:146-147 / :177-178: the reference panics here; report a miss for this subtree
            if (STATS) cnt->kd_plane_miss++;
            cur = NONE;
        }
        if (finished) return true;
        // Leaf: ray.rs:87-99 fold over the leaf's nodes, reference order, strict ends
        if (STATS) cnt->n_leaf++;
        PT_WAVE_COUNT(5);
        bool found = false;
        // The reference's tree puts a node into every leaf its box touches (6.8 references per node on
        // big-scene) and tests all of them. A node whose (padded, outward-rounded) world box the ray's
        // segment [start, end) does not reach cannot report a hit in that range, so it is skipped before
        // the f64 test: same answers, 60 instead of 2 exact tests per ray saved.
        for (int32_t i = 0; i < n.count; i++) {
            const uint32_t item = sc.kd_items[n.first + i];
            if (sc.node_box) {
                const float* b = sc.node_box + 6 * (size_t)(n.first + i);
                if (STATS) cnt->n_bbox++;
                if (!pt_slab_seg_pk(b, b + 3, q, seg0, seg1)) continue;
            }
            PtHit lb; lb.t = end; lb.node = PT_NO_HIT; lb.sub = 0;
            if (pt_test_node<STATS, MESH>(sc, item, ray, start, lb, any, stk, sp, cnt)) {
                best = lb; end = lb.t; found = true;
                if (any) return true;
                // the segment has shrunk: later references of this leaf are culled against the new end
                seg1 = (float)end; seg1 = seg1 + fabsf(seg1) * 2.4e-7f;
            }
        }
        if (found) return true;  // node.rs:153-157: the first side that hits wins
        cur = NONE;
        return false;
    }
};

template <bool STATS, bool MESH = true, class Stack = PtStack>
PT_HD bool pt_trace_kd(const PtSceneView& sc, const PtRay& ray, bool any, PtHit& best, const Stack& stk, PtCounters* cnt) {
    PtKdWalker<MESH> w;
    if (w.begin(sc, ray))
        while (!w.template step<STATS>(sc, ray, any, stk, cnt)) {}
    best = w.best;
    return best.node != PT_NO_HIT;
}
