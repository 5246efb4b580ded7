// Part of pt_trace.h, included after pt_walk_lane.h: the walks with ONE node and ONE stack per wavefront in the flat_scene and hierarchical semantics -
// scalar loads, the packed slab test, pt_descend*, pt_trace_packet* and pt_walk_instance.
#pragma once

// ------------------------------------------------------------------------------------------------
// ONE walk per wavefront (scenes of analytic primitives whose hits spawn no rays: PT_MODE_FLAT_NOMESH / HIER_NOMESH, PARK = 0).
//
// The 64 rays of a wavefront pass through one pixel (or a few) and visit nearly the same nodes - the per-lane walk has 61.8 of
// 64 lanes busy per step on big-scene - so the node index and the stack can be WAVE-UNIFORM instead of per lane:
//  * a node is fetched once per wavefront, through the scalar cache into SGPRs (s_load_dwordx16), and its boxes are scalar
//    operands of the 64 slab tests; the stack is one list in the wavefront's LDS columns; no lane keeps a node index, a stack
//    pointer or a stack column;
//  * a child is entered when ANY lane's ray reaches its box - each lane tests with its own nearest hit so far - and the child
//    most of those lanes call nearer is entered first. Every live lane tests what the wavefront visits (a test below a box its
//    ray misses finds nothing and costs no time: the instruction is issued for the others anyway). The counting build also
//    carries, per stack entry, the mask of the lanes whose rays reach the subtree, and counts a lane's steps and tests only
//    there - what a per-lane walk in the same order would count; carrying the masks in the timed build cost 6 %;
//  * in a leaf the flattened node's record (type, inverse transform) is again one scalar fetch for all lanes.
// The result of a ray does not depend on the order of the walk or on which other candidates are tested (FLAT: nearest hit,
// lowest index on exact ties; HIER: nearest hit, first in depth-first order), so this is a change of schedule, not of results.
// Measured on big-scene: 16.6 -> 19.0 Gray/s with the first version (profiles/r02/notes.md).
// ------------------------------------------------------------------------------------------------
typedef uint32_t pt_u32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t pt_u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t pt_u32x4 __attribute__((ext_vector_type(4)));
// A wave-uniform address as the scalar-register pair the s_load instructions need, wherever the compiler chose to compute it
// (an inline-asm "s" operand that arrives in vector registers is a build error, not a copy).
PT_HD const void* pt_uniform_ptr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long a = (unsigned long long)p;
    const unsigned long long lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return (const void*)((hi << 32) | lo);
#else
    return p;
#endif
}
PT_HD pt_u32x8 pt_sload8(const void* p) {
    pt_u32x8 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    v = *static_cast<const pt_u32x8*>(p);
#endif
    return v;
}
PT_HD pt_u32x4 pt_sload4(const void* p) {
    pt_u32x4 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    v = *static_cast<const pt_u32x4*>(p);
#endif
    return v;
}
PT_HD double pt_f64_of(uint32_t lo, uint32_t hi) {
    union { double d; uint32_t u[2]; } c;
    c.u[0] = lo; c.u[1] = hi;
    return c.d;
}
PT_HD float pt_f32_of(uint32_t u) {
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define PT_UNIFORM_U32(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#define PT_BALLOT(x) __ballot(x)
#define PT_LANE_ID() (threadIdx.x & 63u)
#else
#define PT_UNIFORM_U32(x) ((uint32_t)(x))
#define PT_BALLOT(x) ((x) ? 1ull : 0ull)
#define PT_LANE_ID() 0u
#endif

// 12 doubles (rows 0..2 of a 3x4 matrix) at a wave-uniform address, in one round trip through the scalar cache
PT_HD void pt_sload_mat12(const double* p, double m[12]) {
    pt_u32x16 a;
    pt_u32x8 b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx8 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    a = *reinterpret_cast<const pt_u32x16*>(p);
    b = *reinterpret_cast<const pt_u32x8*>(reinterpret_cast<const char*>(p) + 64);
#endif
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
#pragma unroll
    for (int k = 0; k < 4; k++) m[8 + k] = pt_f64_of(b[2 * k], b[2 * k + 1]);
}
// ... and the 16 bytes that follow the 96 (PtMeshInfo: the box inverse, then {tri_first, tri_count, blas_root, kd_root}), in the same round trip
PT_HD void pt_sload_mat12_x4(const double* p, double m[12], pt_u32x4& tail) {
    pt_u32x16 a;
    pt_u32x8 b;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx16 %0, %3, 0x0\n\ts_load_dwordx8 %1, %3, 0x40\n\ts_load_dwordx4 %2, %3, 0x60\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b), "=&s"(tail) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    a = *reinterpret_cast<const pt_u32x16*>(p);
    b = *reinterpret_cast<const pt_u32x8*>(reinterpret_cast<const char*>(p) + 64);
    tail = *reinterpret_cast<const pt_u32x4*>(reinterpret_cast<const char*>(p) + 96);
#endif
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
#pragma unroll
    for (int k = 0; k < 4; k++) m[8 + k] = pt_f64_of(b[2 * k], b[2 * k + 1]);
}
// May a level whose matrices are the identity be skipped for this ray? ((1 x + 0 y) + 0 z) + 0 is x bit for bit unless x is -0 (which
// the additions turn into +0) or something is not finite (0 times infinity). Wave-uniform: true when no lane's ray has such a component.
PT_HD bool pt_ray_identity_safe(const PtRay& r, bool has_ray) {
    auto odd = [](double v) {
        union { double d; uint32_t u[2]; } c; c.d = v;
        return c.u[1] == 0x80000000u || (c.u[1] & 0x7FF00000u) == 0x7FF00000u;  // -0 (or a negative denormal: taken along) / infinity / NaN
    };
    const bool bad = has_ray && (odd(r.o.x) || odd(r.o.y) || odd(r.o.z) || odd(r.d.x) || odd(r.d.y) || odd(r.d.z));
#if defined(__HIP_DEVICE_COMPILE__)
    return !__any(bad);
#else
    return !bad;
#endif
}
// pt_node_local_ray<true> for a wave-uniform node: the path (hier_rec: one scalar fetch) and every SceneNode's inverse come through the
// scalar cache. identity_ok = pt_ray_identity_safe(ray), worked out once per walk: leading levels that are the identity are skipped then.
PT_HD PtRay pt_node_local_ray_rec(const PtSceneView& sc, uint32_t node, const pt_u32x8& rec, const PtRay& ray, bool identity_ok) {
    PtRay r = ray;
    const uint32_t len = rec[0] & 255u;
    if (len == 255u) {  // a path of more than seven levels
        const uint32_t k0 = PT_UNIFORM_U32(sc.chain_off[node]), k1 = PT_UNIFORM_U32(sc.chain_off[node + 1]);
        for (uint32_t k = k0; k < k1; k++) {
            const uint32_t g = PT_UNIFORM_U32(sc.chain[k]);
            double m[12];
            pt_sload_mat12(sc.g_inv + 12 * (size_t)g, m);
            r = pt_ray_to_local(m, r);
        }
        return r;
    }
    bool untouched = identity_ok;  // the ray is still the world ray
    uint32_t ids[7] = {rec[1], rec[2], rec[3], rec[4], rec[5], rec[6], rec[7]};
    for (uint32_t k = 0; k < len; k++) {
        if (untouched && ((rec[0] >> (8u + k)) & 1u)) continue;
        untouched = false;
        uint32_t g = ids[0];
#pragma unroll
        for (int j = 1; j < 7; j++) g = k == (uint32_t)j ? ids[j] : g;
        double m[12];
        pt_sload_mat12(sc.g_inv + 12 * (size_t)g, m);
        r = pt_ray_to_local(m, r);
    }
    return r;
}
// The same with the node's OWN level's inverse (sc.own_inv, fetched by the caller in the round trip that brought the path record): when every level above the
// node's own is an identity that may be skipped - every reference scene: primitives under an untransformed root - the own level is all there is to apply, and
// no second, dependent fetch is needed (round 4: the hierarchical semantics' leaf tests took two round trips where flat_scene's take one).
PT_HD PtRay pt_node_local_ray_rec_own(const PtSceneView& sc, uint32_t node, const pt_u32x8& rec, const double* own, const PtRay& ray, bool identity_ok) {
    const uint32_t len = rec[0] & 255u;
    if (identity_ok && len >= 1u && len <= 7u) {
        const uint32_t above = (1u << (len - 1u)) - 1u;  // the levels before the last
        if (((rec[0] >> 8) & above) == above) {
            if ((rec[0] >> (8u + len - 1u)) & 1u) return ray;  // the own level is an identity too
            return pt_ray_to_local(own, ray);
        }
    }
    return pt_node_local_ray_rec(sc, node, rec, ray, identity_ok);
}
PT_HD PtRay pt_node_local_ray_uniform(const PtSceneView& sc, uint32_t node, const PtRay& ray, bool identity_ok) {
    pt_u32x8 rec;
    double own[12];
#if defined(__HIP_DEVICE_COMPILE__)
    pt_u32x16 a;
    pt_u32x8 b;
    asm volatile("s_load_dwordx8 %0, %3, 0x0\n\ts_load_dwordx16 %1, %4, 0x0\n\ts_load_dwordx8 %2, %4, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(rec), "=&s"(a), "=&s"(b) : "s"(pt_uniform_ptr(sc.hier_rec + 8 * (size_t)node)), "s"(pt_uniform_ptr(sc.own_inv + 12 * (size_t)node)) : "memory");
#pragma unroll
    for (int k = 0; k < 8; k++) own[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
#pragma unroll
    for (int k = 0; k < 4; k++) own[8 + k] = pt_f64_of(b[2 * k], b[2 * k + 1]);
#else
    rec = pt_sload8(sc.hier_rec + 8 * (size_t)node);
    for (int k = 0; k < 12; k++) own[k] = sc.own_inv[12 * (size_t)node + k];
#endif
    return pt_node_local_ray_rec_own(sc, node, rec, own, ray, identity_ok);
}

// ------------------------------------------------------------------------------------------------
// The slab test of the wave-uniform walks: both children of a node in one go, the node's planes as SCALAR operands.
//
// What limits these walks is the SCALAR unit - one per CU, shared by its sixteen wavefronts (profiles/r03/notes.md: 5.9e9 scalar
// against 4.9e9 vector instructions per big-scene frame with the first version of this test, which let the scalar unit pick the
// entering / leaving plane of every axis) - so everything that can be per-lane arithmetic is, and the scalar side of a step is
// one load, one block of mask logic and the branches.
//
// Per lane and axis two pairs of f32 constants: A = (i, c) applied to the LOWER planes of the children, B = (i, c) applied to the
// UPPER planes. For a positive direction the ray enters a slab through the lower plane, so A holds the "entering" constants
// (i_n, c_n) and B the "leaving" ones (i_f, c_f); for a negative direction it is the other way round. A plane coordinate P gives
// the parameter fma(P, i, c) ~ (P - o) / d; min / max of the two planes' values are the entering / leaving parameters. The
// constants are rounded so that every error makes the overlap LONGER (the walk may only err towards testing more candidates):
//     i0  = rcp((float)d)                        relative error < 2^-22.4 (conversion 2^-24, v_rcp_f32 one ulp)
//     i_n = i0 (1 - 2^-21),  i_f = i0 (1 + 2^-21)    so |i_n| < |1 / d| < |i_f| by at least 2^-22.1 relative, whatever i0's error
//     c_n = fl(-o i_n - w),  c_f = fl(-o i_f + w)    (one fma each from the origin in f32; w = 2.4e-7 relative + 2e-20: more than the
//                                                     origin's conversion and the fma's own rounding - the derivation is with pt_raypk_axis)
// Entering: fma(P, i_n, c_n) <= (P - o) i_n before its one rounding; for a positive parameter T = (P - o) / d that is at most
// T (1 - 2^-22.1), which the fma's rounding (2^-24) cannot lift above T; a negative one stays negative (it is clamped to 0 anyway).
// Leaving: fma(P, i_f, c_f) >= T (1 + 2^-22.1) (1 - 2^-24) >= T for T >= 0; a box with T < 0 lies behind the ray and may be rejected.
// For a box the ray really passes (entering <= leaving, leaving >= 0) the two values come out in that order, so min / max pick
// them correctly; for any other box a wrong order can only turn a rejection into a visit or keep it a rejection.
// An axis the ray is parallel to (|i0| > 1e18 or NaN - which also keeps every product below FLT_MAX for |coordinates| <= 1e18) is
// switched off: A = (0, -inf), B = (0, +inf).
// A step is 6 packed fmas + 20 min / max + 3 compares for both children.
// ------------------------------------------------------------------------------------------------
// Constants of `r` for this lane. *oct (wave-uniform): how the directions of the rays of the lanes in `lanes` relate to the axes -
// bit a set: they all enter slabs of axis a through the UPPER plane (negative direction), clear: through the lower one; PT_OCT_MIXED
// when some axis has rays of both signs among those lanes. Rays through one pixel, or from neighbouring points to one light,
// nearly always share their signs, and then the tree step needs no min / max to tell entering from leaving (pt_slab_pk2).
// Slot `slot` of a mesh leaf (wave-uniform): the triangle's record into scalar registers (dwords 0..15 in `a`, 16 / 17 in b0 / b1), its index returned.
// The record comes from tri_leaf, laid out in slot order - ONE fetch, and a leaf's second triangle sits in the line(s) the first one brought in
// (the slot's index from bvh_items first and then the record it names were two dependent fetches). The walks test triangles from their edge records (tri_e).
#define PT_TRI_HIT pt_triangle_hit_e
// (from a base address the caller may hold in scalar registers - pt_pin_ptr(sc.tri_leaf) -: read through the scene view it was fetched again for every triangle)
PT_HD uint32_t pt_load_leaf_triangle_at(const double* tri_leaf, uint32_t slot, pt_u32x16& a, uint32_t& b0, uint32_t& b1) {
    const double* rec = tri_leaf + 10 * (size_t)slot;
#if defined(__HIP_DEVICE_COMPILE__)
    pt_u32x4 b;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b) : "s"(pt_uniform_ptr(rec)) : "memory");
    b0 = b[0]; b1 = b[1];
    return b[2];
#else
    a = *reinterpret_cast<const pt_u32x16*>(rec);
    b0 = reinterpret_cast<const uint32_t*>(rec)[16]; b1 = reinterpret_cast<const uint32_t*>(rec)[17];
    return reinterpret_cast<const uint32_t*>(rec)[18];
#endif
}
PT_HD uint32_t pt_load_leaf_triangle(const PtSceneView& sc, uint32_t slot, pt_u32x16& a, uint32_t& b0, uint32_t& b1) {
    return pt_load_leaf_triangle_at(sc.tri_leaf, slot, a, b0, b1);
}
#define PT_OCT_MIXED 8
PT_HD PtRayPk pt_raypk(const PtRay& r, bool lanes, int* oct) {
    PtRayPk q;
    const int sx = pt_raypk_axis(r.o.x, r.d.x, &q.a[0], &q.b[0]);
    const int sy = pt_raypk_axis(r.o.y, r.d.y, &q.a[1], &q.b[1]);
    const int sz = pt_raypk_axis(r.o.z, r.d.z, &q.a[2], &q.b[2]);
    const bool nx = PT_BALLOT(lanes && sx == 2) != 0ull, px = PT_BALLOT(lanes && sx == 1) != 0ull;
    const bool ny = PT_BALLOT(lanes && sy == 2) != 0ull, py = PT_BALLOT(lanes && sy == 1) != 0ull;
    const bool nz = PT_BALLOT(lanes && sz == 2) != 0ull, pz = PT_BALLOT(lanes && sz == 1) != 0ull;
    // A lane with a switched-off axis holds A = (0, -inf), B = (0, +inf) there: "entering through the lower plane". Under an octant
    // whose bit for that axis is set pt_slab_pk2 would read B as the entering value (+inf) and reject every box for that lane - its ray
    // would silently miss the scene (level cameras with centre sampling: a whole row / column of pixels). Such a wavefront takes the
    // per-lane form, where min / max sort the pair whatever the octant.
    const bool off = PT_BALLOT(lanes && (sx == 0 || sy == 0 || sz == 0)) != 0ull;
    *oct = (off || (nx && px) || (ny && py) || (nz && pz)) ? PT_OCT_MIXED : ((nx ? 1 : 0) | (ny ? 2 : 0) | (nz ? 4 : 0));
    return q;
}
PT_HD pt_f32x2 pt_pair_f32(uint32_t a, uint32_t b) { pt_f32x2 v; v.x = pt_f32_of(a); v.y = pt_f32_of(b); return v; }
// packed fma with per-lane constants (i, c) broadcast to both halves: (p.x i + c, p.y i + c)
PT_HD pt_f32x2 pt_pk_fma_bcast(pt_f32x2 planes, pt_f32x2 ic) {
#if defined(__HIP_DEVICE_COMPILE__)
    pt_f32x2 r;
    // src1 = ic.x for both halves (op_sel 0 / op_sel_hi 0), src2 = ic.y for both halves (op_sel 1 / op_sel_hi 1)
    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "s"(planes), "v"(ic));
    return r;
#else
    pt_f32x2 r;
    r.x = __builtin_fmaf(planes.x, ic.x, ic.y); r.y = __builtin_fmaf(planes.y, ic.x, ic.y);
    return r;
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_FCMP_LE(a, b) __builtin_amdgcn_fcmpf((a), (b), 5)  // ordered <=, as a lane mask
#define PT_FCMP_LT(a, b) __builtin_amdgcn_fcmpf((a), (b), 4)
#else
#define PT_FCMP_LE(a, b) (((a) <= (b)) ? 1ull : 0ull)
#define PT_FCMP_LT(a, b) (((a) < (b)) ? 1ull : 0ull)
#endif
// min / max as single instructions: fmaxf / fminf on a value that comes out of inline asm make the compiler canonicalise it first
// (one v_max x, x per operand - twelve extra instructions per tree step)
PT_HD float pt_max2_raw(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
#else
    return fmaxf(a, b);
#endif
}
PT_HD float pt_min2_raw(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r;
#else
    return fminf(a, b);
#endif
}
PT_HD float pt_max3_zero_raw(float a, float b) {  // max(a, b, 0)
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_max3_f32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b)); return r;
#else
    return fmaxf(fmaxf(a, b), 0.0f);
#endif
}
PT_HD float pt_max3_raw(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
#else
    return fmaxf(fmaxf(a, b), c);
#endif
}
PT_HD float pt_min3_raw(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r;
#else
    return fminf(fminf(a, b), c);
#endif
}
// Both child boxes of node record `v` (PtBvhNode as 16 dwords in scalar registers) against every lane's ray over [0, tm].
// Out: masks of the lanes whose rays reach child 0 / child 1, and of those that reach child 1 strictly before child 0.
// OCT (see pt_raypk): with wave-uniform signs the entering value of an axis is the lower planes' (bit clear) or the upper planes'
// (bit set) - known at compile time, 6 packed fmas + 8 min / max + 3 compares; PT_OCT_MIXED: min / max of the two per lane (+ 12).
// NEAR: the lane's segment starts at t0 > 0 (the k-d semantics' nested mesh walks: a leaf's range [start, end)) - the entering value is
// clamped there instead of at 0, the same instruction with a register in place of the constant.
template <int OCT, bool NEAR = false>
PT_HD void pt_slab_pk2(const pt_u32x16& v, const PtRayPk& q, float tm, unsigned long long* m0, unsigned long long* m1, unsigned long long* one_first, float t0 = 0.0f) {
    const pt_f32x2 ax = pt_pk_fma_bcast(pt_pair_f32(v[0], v[1]), q.a[0]), ay = pt_pk_fma_bcast(pt_pair_f32(v[2], v[3]), q.a[1]), az = pt_pk_fma_bcast(pt_pair_f32(v[4], v[5]), q.a[2]);
    const pt_f32x2 bx = pt_pk_fma_bcast(pt_pair_f32(v[6], v[7]), q.b[0]), by = pt_pk_fma_bcast(pt_pair_f32(v[8], v[9]), q.b[1]), bz = pt_pk_fma_bcast(pt_pair_f32(v[10], v[11]), q.b[2]);
    float tn0, tn1, tf0, tf1;
    if (OCT == PT_OCT_MIXED) {
        if (NEAR) {
            tn0 = pt_max3_raw(pt_max2_raw(pt_min2_raw(ax.x, bx.x), pt_min2_raw(ay.x, by.x)), pt_min2_raw(az.x, bz.x), t0);
            tn1 = pt_max3_raw(pt_max2_raw(pt_min2_raw(ax.y, bx.y), pt_min2_raw(ay.y, by.y)), pt_min2_raw(az.y, bz.y), t0);
        } else {
            tn0 = pt_max3_zero_raw(pt_max2_raw(pt_min2_raw(ax.x, bx.x), pt_min2_raw(ay.x, by.x)), pt_min2_raw(az.x, bz.x));
            tn1 = pt_max3_zero_raw(pt_max2_raw(pt_min2_raw(ax.y, bx.y), pt_min2_raw(ay.y, by.y)), pt_min2_raw(az.y, bz.y));
        }
        tf0 = pt_min3_raw(pt_min2_raw(pt_max2_raw(ax.x, bx.x), pt_max2_raw(ay.x, by.x)), pt_max2_raw(az.x, bz.x), tm);
        tf1 = pt_min3_raw(pt_min2_raw(pt_max2_raw(ax.y, bx.y), pt_max2_raw(ay.y, by.y)), pt_max2_raw(az.y, bz.y), tm);
    } else {
        const pt_f32x2 ex = (OCT & 1) ? bx : ax, lx = (OCT & 1) ? ax : bx;  // entering / leaving values per axis, both children
        const pt_f32x2 ey = (OCT & 2) ? by : ay, ly = (OCT & 2) ? ay : by;
        const pt_f32x2 ez = (OCT & 4) ? bz : az, lz = (OCT & 4) ? az : bz;
        if (NEAR) { tn0 = pt_max3_raw(pt_max2_raw(ex.x, ey.x), ez.x, t0); tn1 = pt_max3_raw(pt_max2_raw(ex.y, ey.y), ez.y, t0); }
        else { tn0 = pt_max3_zero_raw(pt_max2_raw(ex.x, ey.x), ez.x); tn1 = pt_max3_zero_raw(pt_max2_raw(ex.y, ey.y), ez.y); }
        tf0 = pt_min3_raw(pt_min2_raw(lx.x, ly.x), lz.x, tm); tf1 = pt_min3_raw(pt_min2_raw(lx.y, ly.y), lz.y, tm);
    }
    *m0 = PT_FCMP_LE(tn0, tf0);
    *m1 = PT_FCMP_LE(tn1, tf1);
    *one_first = PT_FCMP_LT(tn1, tn0);
}
// The same test handing out the entering parameters as well (pt_descend_mesh's branching form works out which child goes first only where both are reached).
template <int OCT, bool NEAR = false>
PT_HD void pt_slab_pk2_t(const pt_u32x16& v, const PtRayPk& q, float tm, unsigned long long* m0, unsigned long long* m1, float* tn0_out, float* tn1_out, float t0 = 0.0f) {
    const pt_f32x2 ax = pt_pk_fma_bcast(pt_pair_f32(v[0], v[1]), q.a[0]), ay = pt_pk_fma_bcast(pt_pair_f32(v[2], v[3]), q.a[1]), az = pt_pk_fma_bcast(pt_pair_f32(v[4], v[5]), q.a[2]);
    const pt_f32x2 bx = pt_pk_fma_bcast(pt_pair_f32(v[6], v[7]), q.b[0]), by = pt_pk_fma_bcast(pt_pair_f32(v[8], v[9]), q.b[1]), bz = pt_pk_fma_bcast(pt_pair_f32(v[10], v[11]), q.b[2]);
    float tn0, tn1, tf0, tf1;
    if (OCT == PT_OCT_MIXED) {
        if (NEAR) {
            tn0 = pt_max3_raw(pt_max2_raw(pt_min2_raw(ax.x, bx.x), pt_min2_raw(ay.x, by.x)), pt_min2_raw(az.x, bz.x), t0);
            tn1 = pt_max3_raw(pt_max2_raw(pt_min2_raw(ax.y, bx.y), pt_min2_raw(ay.y, by.y)), pt_min2_raw(az.y, bz.y), t0);
        } else {
            tn0 = pt_max3_zero_raw(pt_max2_raw(pt_min2_raw(ax.x, bx.x), pt_min2_raw(ay.x, by.x)), pt_min2_raw(az.x, bz.x));
            tn1 = pt_max3_zero_raw(pt_max2_raw(pt_min2_raw(ax.y, bx.y), pt_min2_raw(ay.y, by.y)), pt_min2_raw(az.y, bz.y));
        }
        tf0 = pt_min3_raw(pt_min2_raw(pt_max2_raw(ax.x, bx.x), pt_max2_raw(ay.x, by.x)), pt_max2_raw(az.x, bz.x), tm);
        tf1 = pt_min3_raw(pt_min2_raw(pt_max2_raw(ax.y, bx.y), pt_max2_raw(ay.y, by.y)), pt_max2_raw(az.y, bz.y), tm);
    } else {
        const pt_f32x2 ex = (OCT & 1) ? bx : ax, lx = (OCT & 1) ? ax : bx;
        const pt_f32x2 ey = (OCT & 2) ? by : ay, ly = (OCT & 2) ? ay : by;
        const pt_f32x2 ez = (OCT & 4) ? bz : az, lz = (OCT & 4) ? az : bz;
        if (NEAR) { tn0 = pt_max3_raw(pt_max2_raw(ex.x, ey.x), ez.x, t0); tn1 = pt_max3_raw(pt_max2_raw(ex.y, ey.y), ez.y, t0); }
        else { tn0 = pt_max3_zero_raw(pt_max2_raw(ex.x, ey.x), ez.x); tn1 = pt_max3_zero_raw(pt_max2_raw(ex.y, ey.y), ez.y); }
        tf0 = pt_min3_raw(pt_min2_raw(lx.x, ly.x), lz.x, tm); tf1 = pt_min3_raw(pt_min2_raw(lx.y, ly.y), lz.y, tm);
    }
    *m0 = PT_FCMP_LE(tn0, tf0);
    *m1 = PT_FCMP_LE(tn1, tf1);
    *tn0_out = tn0; *tn1_out = tn1;
}
// a lane's exclusive range end as the f32 the slab test compares with, rounded up (inf stays inf)
PT_HD float pt_tmax32(double t) { float tm = (float)t; return tm + fabsf(tm) * 2.4e-7f; }

// The bound a lane ENTERS the two wavefront walks of the flat_scene and hierarchical semantics with (pt_trace_packet_walk, pt_trace_packet_mesh): best.t, and
// tm, its f32 image for the slab tests. Every pass but one starts a walk over [EPSILON, inf): these defaults, which expand to the text that stood here before
// the seam. The bounded-segment pass (pt_segments_inst.hip) defines both BEFORE its includes so that its copy of the walks keeps the best.t the lane came in
// with - its t_max - and prunes with it from the first box on; pt_cand_end / pt_cand_end_in then give every candidate [EPSILON, t_max). A macro and not a
// template parameter, because editing the walks' templates reorders every render object's code.
//
// The third macro is the test of a KDMesh instance's own triangle k-d tree in pt_trace_packet_mesh. Its side classification reads the END of the range it is given
// (pt_kdmesh_hit: `end - PT_EPSILON`, node.rs:121), so a walk handed a caller's bound can lose a hit just inside that bound which the walk over [EPSILON, inf)
// finds. The bounded-segment pass promises the unbounded result, filtered - here as in the scene-level k-d semantics - and uses pt_kdmesh_hit_filtered instead.
// The fourth is the range end of a Mesh instance's box test there (bounding_box.rs:104-116, a cube hit in [EPSILON, end)): the box's entry parameter and a
// triangle's t are rounded differently, so where a triangle lies IN a face of its mesh's box a bound one ulp behind the triangle can lie in front of the box. The
// bounded-segment pass tests the box over [EPSILON, inf) while the lane has found nothing; the triangles get the bound, whose comparison with their t is exact.
#ifndef PT_WALK_ENTRY_T
#define PT_WALK_ENTRY_T(best) INFINITY
#define PT_WALK_ENTRY_TM(best) INFINITY
#define PT_WALK_KDMESH_HIT(STATS, HIER, sc, mi, lr, best, node, lane_stk, t, tri, cnt) pt_kdmesh_hit<STATS>(sc, mi, lr, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, node, 0), lane_stk, 0, t, tri, cnt)
#define PT_WALK_MESH_BOX_END(HIER, sc, best, node) pt_cand_end_in<HIER>(sc, best, node, 0)
#endif

// pt_kdmesh_hit for a walk that was entered with a bound (best.t = t_max, best.node = PT_NO_HIT): as long as nothing is found, best.t is no hit and the mesh's tree
// gets the range an unbounded walk would give it, [EPSILON, inf); its hit then counts iff it lies in front of the bound. Once something is found best.t is a hit
// like any other.
template <bool STATS, bool HIER, class Stack>
PT_HD bool pt_kdmesh_hit_filtered(const PtSceneView& sc, const PtMeshInfo& m, const PtRay& lr, const PtHit& best, uint32_t node, const Stack& stk, double* t, uint32_t* tri,
                                  PtCounters* cnt) {
    const bool open = best.node == PT_NO_HIT;
    if (!pt_kdmesh_hit<STATS>(sc, m, lr, PT_EPSILON, open ? (double)INFINITY : pt_cand_end_in<HIER>(sc, best, node, 0), stk, 0, t, tri, cnt)) return false;
    return !open || *t < best.t;
}

// The scalar side of a step in one block: which children the wavefront enters (code 0: neither, 1: child 0 only, 2: child 1
// only, 3: both), which one first (`near`: the one the majority of the lanes that reach a child enter first; with a single
// child reached that is that child) and which one waits on the stack (`far`, meaningful for code 3).
// m0 / m1: lanes reaching child 0 / 1; one_first: lanes reaching child 1 before child 0; lanes: the lanes that count.
PT_HD uint32_t pt_step_decide(unsigned long long* m0_io, unsigned long long* m1_io, unsigned long long one_first, unsigned long long lanes, uint32_t c0, uint32_t c1,
                              uint32_t* near, uint32_t* far) {
    unsigned long long m0 = *m0_io, m1 = *m1_io;
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t code, h1, n_sf, n_u, nr, fr;
    unsigned long long t;
    asm volatile(
        "s_and_b64 %[m0], %[m0], %[lanes]\n\t"
        "s_cselect_b32 %[code], 1, 0\n\t"
        "s_and_b64 %[m1], %[m1], %[lanes]\n\t"
        "s_cselect_b32 %[h1], 2, 0\n\t"
        "s_orn2_b64 %[t], %[of], %[m0]\n\t"      // lanes that reach child 1 first: m1 & (one_first | ~m0)
        "s_and_b64 %[t], %[t], %[m1]\n\t"
        "s_bcnt1_i32_b64 %[nsf], %[t]\n\t"
        "s_or_b64 %[t], %[m0], %[m1]\n\t"
        "s_bcnt1_i32_b64 %[nu], %[t]\n\t"
        "s_lshl_b32 %[nsf], %[nsf], 1\n\t"
        "s_cmp_gt_u32 %[nsf], %[nu]\n\t"         // most of them: child 1 first
        "s_cselect_b32 %[nr], %[c1], %[c0]\n\t"
        "s_cselect_b32 %[fr], %[c0], %[c1]\n\t"
        "s_or_b32 %[code], %[code], %[h1]"
        : [code] "=&s"(code), [h1] "=&s"(h1), [t] "=&s"(t), [nsf] "=&s"(n_sf), [nu] "=&s"(n_u), [nr] "=&s"(nr), [fr] "=&s"(fr), [m0] "+s"(m0), [m1] "+s"(m1)
        : [of] "s"(one_first), [lanes] "s"(lanes), [c0] "s"(c0), [c1] "s"(c1)
        : "scc");
    *near = nr; *far = fr; *m0_io = m0; *m1_io = m1;
    return code;
#else
    m0 &= lanes; m1 &= lanes;
    const unsigned long long second_first = m1 & (one_first | ~m0);
    const bool swap = __builtin_popcountll(second_first) * 2 > __builtin_popcountll(m0 | m1);
    *near = swap ? c1 : c0; *far = swap ? c0 : c1; *m0_io = m0; *m1_io = m1;
    return (m0 ? 1u : 0u) | (m1 ? 2u : 0u);
#endif
}
// node record `index` of the tree array at `base` (64-byte records): one scalar load with a 32-bit byte offset
PT_HD pt_u32x16 pt_sload_node(const void* base, uint32_t index) {
    pt_u32x16 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pt_uniform_ptr(base)), "s"(index << 6) : "memory");
#else
    v = static_cast<const pt_u32x16*>(base)[index];
#endif
    return v;
}

// One flattened node against every participating lane's ray; `node` is wave-uniform.
// EYE (flat_scene semantics, primary rays): every lane's origin is the camera's eye, the same in every lane, item and wavefront of the launch. The same two
// scalar loads then read the node's record of the launch's eye table `eye_tab` (pt_eye_table_kernel, pt_api.hip) instead of sc.inv: the inverse with its
// translation column replaced by pt_xform_point(inverse, eye) - the local origin, bit for bit what every lane worked out per leaf test (9 f64 products and 9 sums
// on six vector registers that no longer live through the walk); ray.o is not read. The direction is transformed as before.
template <bool STATS, bool HIER, bool EYE = false>
PT_HD bool pt_test_node_uniform(const PtSceneView& sc, uint32_t node, const PtRay& ray, bool identity_ok, PtHit& best, PtCounters* cnt, const double* eye_tab = nullptr) {
    static_assert(!(EYE && HIER), "the eye table holds composed inverses: flat_scene semantics only");
    // the node's record in one round trip through the scalar cache: {type, data, flags, material} and rows 0..2 of its inverse
    pt_u32x4 info;
    pt_u32x16 a;  // doubles 0..7 of the 3x4 inverse
    pt_u32x8 b;   // doubles 8..11
    const void* info_ptr = sc.info + 4 * (size_t)node;
    const void* rec = (EYE ? eye_tab : sc.inv) + 12 * (size_t)node;
#if defined(__HIP_DEVICE_COMPILE__)
    pt_u32x8 hrec;  // HIER: the node's path record
    if (HIER) {  // ... the node's path record (hier_rec) and the inverse of its OWN level instead of a composed inverse
        asm volatile("s_load_dwordx4 %0, %4, 0x0\n\ts_load_dwordx8 %1, %5, 0x0\n\ts_load_dwordx16 %2, %6, 0x0\n\ts_load_dwordx8 %3, %6, 0x40\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(info), "=&s"(hrec), "=&s"(a), "=&s"(b)
                     : "s"(pt_uniform_ptr(info_ptr)), "s"(pt_uniform_ptr(sc.hier_rec + 8 * (size_t)node)), "s"(pt_uniform_ptr(sc.own_inv + 12 * (size_t)node)) : "memory");
    } else {
        asm volatile("s_load_dwordx4 %0, %3, 0x0\n\ts_load_dwordx16 %1, %4, 0x0\n\ts_load_dwordx8 %2, %4, 0x40\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(info), "=&s"(a), "=&s"(b) : "s"(pt_uniform_ptr(info_ptr)), "s"(pt_uniform_ptr(rec)) : "memory");
    }
#else
    info = *static_cast<const pt_u32x4*>(info_ptr);
    pt_u32x8 hrec;
    if (HIER) {
        hrec = *reinterpret_cast<const pt_u32x8*>(sc.hier_rec + 8 * (size_t)node);
        rec = sc.own_inv + 12 * (size_t)node;
    }
    a = *static_cast<const pt_u32x16*>(rec);
    b = *reinterpret_cast<const pt_u32x8*>(static_cast<const char*>(rec) + 64);
#endif
    const uint32_t type = info[0], data = info[1];
    PtRay local;
    {
        double m[12];
#pragma unroll
        for (int k = 0; k < 8; k++) m[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
#pragma unroll
        for (int k = 0; k < 4; k++) m[8 + k] = pt_f64_of(b[2 * k], b[2 * k + 1]);
        if (HIER) local = pt_node_local_ray_rec_own(sc, node, hrec, m, ray, identity_ok);
        else if (EYE) { local.o = pt_v3(m[3], m[7], m[11]); local.d = pt_xform_dir(m, 4, ray.d); }
        else local = pt_ray_to_local(m, ray);
    }
    if (STATS) cnt->n_analytic++;
    double t;
    uint32_t part = 0;
    bool hit;
    if (type == PT_TRIANGLE) {  // stand-alone triangle, stored after the mesh triangles
        double beta, gamma;
        if (STATS) cnt->n_tri++;
        hit = pt_triangle_hit(sc.tri_v + 9 * (size_t)data, local, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, node, data), &t, &beta, &gamma);
        part = data;
    } else {
        hit = pt_unit_prim_hit(type, local, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, node, 0), &t, &part);
    }
    if (!hit) return false;
    best.t = t; best.node = node; best.sub = part;
    return true;
}

// Down from inner node `cur` to the next leaf: ONE loop with one way out - `cur` becomes a leaf reference, or PT_REF_EMPTY when
// nothing is left (or the stack overflowed: `overflowed`). Every `return` or `break` in here would cost scalar instructions in
// EVERY step (the compiler turns the exits into flags it sets and tests), and the CU's one scalar unit is what these steps wait
// for. `lanes`: the lanes whose rays count; W words per stack entry (3 in the counting build: the node and the mask of the lanes
// that reach it, which `in` follows).
template <bool STATS, int OCT>
PT_HD void pt_descend(const PtBvhNode* bvh, const PtRayPk& q, float tm, unsigned long long lanes, unsigned long long self, uint32_t& cur, int& sp, unsigned long long& in,
                      bool& overflowed, uint32_t* wstack, int words, uint32_t& pops, PtCounters* cnt) {
    constexpr int W = STATS ? 3 : 1;
#if defined(__HIP_DEVICE_COMPILE__)  // (round 3's single block for every case, below, serves the counting build and the host; measured against this one in profiles/r05/notes.md section 6)
    if (!STATS) {  // (see pt_descend_mesh: the common case - one child reached - in six scalar instructions; vote, push and pop behind branches)
        while (!(cur & PT_REF_LEAF)) {
            const pt_u32x16 v = pt_sload_node(bvh, cur);
            PT_WAVE_COUNT(4);
            unsigned long long m0, m1;
            float tn0, tn1;
            pt_slab_pk2_t<OCT>(v, q, tm, &m0, &m1, &tn0, &tn1);
            uint32_t next, both, f0;
            asm volatile(
                "s_and_b64 %[m0], %[m0], %[lanes]\n\t"
                "s_cselect_b32 %[next], %[c0], %[pop]\n\t"
                "s_cselect_b32 %[f0], 1, 0\n\t"
                "s_and_b64 %[m1], %[m1], %[lanes]\n\t"
                "s_cselect_b32 %[next], %[c1], %[next]\n\t"
                "s_cselect_b32 %[both], %[f0], 0"
                : [next] "=&s"(next), [both] "=&s"(both), [f0] "=&s"(f0), [m0] "+s"(m0), [m1] "+s"(m1)
                : [lanes] "s"(lanes), [c0] "s"(v[12]), [c1] "s"(v[13]), [pop] "s"(PT_REF_POP)
                : "scc");
            if (both) {
                const unsigned long long second_first = m1 & (PT_FCMP_LT(tn1, tn0) | ~m0);
                const bool swap = __builtin_popcountll(second_first) * 2 > __builtin_popcountll(m0 | m1);
                const uint32_t near = swap ? v[13] : v[12], far = swap ? v[12] : v[13];
                if (sp + 1 <= words) { wstack[sp] = far; sp++; next = near; }
                else { overflowed = true; next = PT_REF_EMPTY; }
            } else if (next == PT_REF_POP) {  // neither: the next pending subtree
                if (sp > 0) {
                    sp--;
                    next = PT_UNIFORM_U32(wstack[sp]);
                } else {
                    overflowed = overflowed || sp > 0;
                    next = PT_REF_EMPTY;
                }
            }
            cur = next;
        }
        return;
    }
#endif
    while (!(cur & PT_REF_LEAF)) {
        const pt_u32x16 v = pt_sload_node(bvh, cur);
        PT_WAVE_COUNT(4);
        const unsigned long long mine = STATS ? (lanes & in) : lanes;
        if (STATS && (mine & self)) cnt->n_inner++;
        unsigned long long m0, m1, one_first;
        pt_slab_pk2<OCT>(v, q, tm, &m0, &m1, &one_first);
        uint32_t near, far;
        const uint32_t code = pt_step_decide(&m0, &m1, one_first, mine, v[12], v[13], &near, &far);
        uint32_t next = near;
        if (STATS) in = (code == 3u ? near == v[12] : code == 1u) ? m0 : m1;
        if (code == 3u) {  // both: the other one waits on the stack
            if (sp + W <= words) {
                wstack[sp] = far;
                if (STATS) { const unsigned long long far_mask = far == v[12] ? m0 : m1; wstack[sp + 1] = (uint32_t)far_mask; wstack[sp + 2] = (uint32_t)(far_mask >> 32); }
                sp += W;
            } else {
                overflowed = true; next = PT_REF_EMPTY;
            }
        }
        if (code == 0u) {  // neither: the next pending subtree
            // (no watchdog on these pops: the counter inside the mesh-free walk's hand-tuned step cost 3.5 % on big-scene - 15 more spilled scalar
            // registers, profiles/r04/notes.md)
            if (sp > 0) {
                sp -= W;
                next = PT_UNIFORM_U32(wstack[sp]);
                if (STATS) in = (unsigned long long)PT_UNIFORM_U32(wstack[sp + 1]) | ((unsigned long long)PT_UNIFORM_U32(wstack[sp + 2]) << 32);
            } else {
                overflowed = overflowed || sp > 0;
                next = PT_REF_EMPTY;
            }
        }
        cur = next;
    }
}

// The same inside the two-level walk of scenes with mesh instances: PT_REF_POP when neither child is reached (the caller pops: the
// instance's part of the stack may be used up), PT_REF_EMPTY when the stack overflowed.
template <bool STATS, int OCT, bool NEAR = false>
PT_HD void pt_descend_mesh(const PtBvhNode* bvh, const PtRayPk& q, float tm, unsigned long long lanes, bool counts, uint32_t& cur, int& sp, uint32_t* wstack, int words,
                           PtCounters* cnt, float t0 = 0.0f) {
#if defined(__HIP_DEVICE_COMPILE__)  // (round 3's single block for every case, below, serves the counting build and the host; measured against this one in profiles/r05/notes.md section 6)
    {
        // Round 5: the step's scalar side by CASES instead of one straight block of mask arithmetic for all of them. About half of the steps reach one child
        // only (or none); for those the majority vote, the code word and the push logic are never issued - the walk is bound by the scalar unit's issue
        // rate, not by the fetches (profiles/r05/notes.md section 6: two levels per fetch lost 10 %, eight scalar instructions fewer per step won 5 %).
        // Same children, same order, same pushes as the single block (the counting build still runs that one).
        while (!(cur & PT_REF_LEAF)) {
            const pt_u32x16 v = pt_sload_node(bvh, cur);
            PT_WAVE_COUNT(4);
            if (STATS && counts) cnt->n_inner++;
            unsigned long long m0, m1;
            float tn0, tn1;
            pt_slab_pk2_t<OCT, NEAR>(v, q, tm, &m0, &m1, &tn0, &tn1, t0);
            // The scalar side of the common case in six instructions: the masks cut down to the participating lanes, `next` = the one child reached (or
            // PT_REF_POP), `both` = 1 when both are - only then the vote and the push are issued.
            uint32_t next, both, f0;
            asm volatile(
                "s_and_b64 %[m0], %[m0], %[lanes]\n\t"
                "s_cselect_b32 %[next], %[c0], %[pop]\n\t"
                "s_cselect_b32 %[f0], 1, 0\n\t"
                "s_and_b64 %[m1], %[m1], %[lanes]\n\t"
                "s_cselect_b32 %[next], %[c1], %[next]\n\t"
                "s_cselect_b32 %[both], %[f0], 0"
                : [next] "=&s"(next), [both] "=&s"(both), [f0] "=&s"(f0), [m0] "+s"(m0), [m1] "+s"(m1)
                : [lanes] "s"(lanes), [c0] "s"(v[12]), [c1] "s"(v[13]), [pop] "s"(PT_REF_POP)
                : "scc");
            if (both) {  // the one most of the lanes that reach a child enter first (pt_step_decide's vote)
                const unsigned long long second_first = m1 & (PT_FCMP_LT(tn1, tn0) | ~m0);
                const bool swap = __builtin_popcountll(second_first) * 2 > __builtin_popcountll(m0 | m1);
                const uint32_t near = swap ? v[13] : v[12], far = swap ? v[12] : v[13];
                if (sp + 1 <= words) { wstack[sp] = far; sp++; next = near; }
                else next = PT_REF_EMPTY;
            }
            cur = next;
        }
        return;
    }
#endif
    while (!(cur & PT_REF_LEAF)) {
        const pt_u32x16 v = pt_sload_node(bvh, cur);
        PT_WAVE_COUNT(4);
        if (STATS && counts) cnt->n_inner++;
        unsigned long long m0, m1, one_first;
        pt_slab_pk2<OCT, NEAR>(v, q, tm, &m0, &m1, &one_first, t0);
        uint32_t near, far;
        const uint32_t code = pt_step_decide(&m0, &m1, one_first, lanes, v[12], v[13], &near, &far);
        uint32_t next = near;
        if (code == 3u) {
            if (sp + 1 <= words) { wstack[sp] = far; sp++; }
            else next = PT_REF_EMPTY;
        }
        if (code == 0u) next = PT_REF_POP;
        cur = next;
    }
}

// wstack: the wavefront's own stack in LDS, `wwords` 32-bit words, linear. `live` = false: the lane's (shadow) ray is answered
// already - its `best` is kept and it takes no part in the walk, while everything wave-wide (octant, identity levels) still follows
// `has_ray`, as if it did (pt_trace_packet's occluder test). EYE: a walk of primary rays whose leaf tests take the local origin from `eye_tab`
// (pt_test_node_uniform); ray.o is read for the slab test's constants at the top and not after.
template <bool STATS, bool HIER, bool EYE = false>
PT_HD void pt_trace_packet_walk(const PtSceneView& sc, const PtRay& ray, bool has_ray, bool any, PtHit& best, uint32_t* wstack, int wwords,
                                unsigned int* overflow, PtCounters* cnt, bool live = true, const double* eye_tab = nullptr) {
    if (has_ray && live) { best.t = PT_WALK_ENTRY_T(best); best.node = PT_NO_HIT; best.sub = 0; }
    if (sc.n_nodes == 0 || sc.tlas_root == PT_REF_EMPTY) return;
    const unsigned long long self = 1ull << PT_LANE_ID();
    bool alive = has_ray && live;       // the lane still wants candidates (a shadow ray stops at its first hit)
    unsigned long long amask = PT_BALLOT(alive);  // the same as a wave-uniform mask: the slab test's results are masks, never per-lane booleans
    unsigned long long in = ~0ull;      // wave-uniform: lanes whose rays reach the current node's box
    int oct;
    const PtRayPk q = pt_raypk(ray, has_ray, &oct);
    const bool identity_ok = HIER && pt_ray_identity_safe(ray, has_ray);  // (wave-uniform) levels of a path that are the identity may be skipped
    float tm = PT_WALK_ENTRY_TM(best);                 // best.t as the f32 bound of the slab test, rounded up; follows best.t
    uint32_t cur = PT_UNIFORM_U32(sc.tlas_root);
    int sp = 0;                          // words on the stack
    constexpr int W = STATS ? 3 : 1;     // per entry: the node, and in the counting build the mask of the lanes that reach it
    const int words = wwords < W * sc.stack_cap ? wwords : W * sc.stack_cap;  // scene.stack_cap entries, if the LDS region holds them
    // (No watchdog in THIS walk - the walks of scenes with meshes and the k-d walk count their pending subtrees, where it measures nothing: three scalar
    // instructions per pending subtree cost the headline 1.1 % (c16 / c22), and what they buy is little - a walk of a valid tree ends by itself (a node is
    // entered at most once, pushes are bounded by the stack), and the one hang this code base has seen was not in a walk (profiles/r04/notes.md).)
    uint32_t pops = 0;                   // (stays 0; what pt_descend's signature and the overflow code below still carry of the watchdog)
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(pops));       // (kept in a scalar register: left to itself the compiler parks it in a vector register's lane and spills four more of those)
#endif
    for (;;) {
        bool overflowed = false;         // the stack overflowed inside pt_descend
        if (!(cur & PT_REF_LEAF)) {
            const unsigned long long mine = amask;
            switch (STATS ? PT_OCT_MIXED : oct) {  // the counting build always takes the per-lane form (its images are compared with the plain build's)
            case 0: pt_descend<STATS, 0>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 1: pt_descend<STATS, 1>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 2: pt_descend<STATS, 2>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 3: pt_descend<STATS, 3>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 4: pt_descend<STATS, 4>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 5: pt_descend<STATS, 5>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 6: pt_descend<STATS, 6>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            case 7: pt_descend<STATS, 7>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            default: pt_descend<STATS, PT_OCT_MIXED>(sc.bvh, q, tm, mine, self, cur, sp, in, overflowed, wstack, words, pops, cnt); break;
            }
        }
        if (cur == PT_REF_EMPTY) {
            if (overflowed) {
#if defined(__HIP_DEVICE_COMPILE__)
                if (overflow) atomicOr(overflow, pops > PT_WALK_POPS_MAX ? 4u : 1u);  // 4: the watchdog
#endif
                if (STATS) cnt->stack_overflow++;
                if (has_ray) best.node = PT_NO_HIT;
            }
            return;
        }
        const uint32_t first = (cur & ~PT_REF_LEAF) >> 3, count = (cur & 7u) + 1u;
        PT_WAVE_COUNT(5);
        {
        PT_CYC_BEGIN();
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t node = sc.tlas_direct ? first : PT_UNIFORM_U32(sc.bvh_items[first + i]);
            if (alive && (!STATS || (in & self))) {
                if (STATS) cnt->n_leaf++;
                if (pt_test_node_uniform<STATS, HIER, EYE>(sc, node, ray, identity_ok, best, cnt, eye_tab)) {
                    tm = pt_tmax32(best.t);
                    if (any) alive = false;
                }
            }
        }
        PT_CYC_END(5);
        }
        amask = PT_BALLOT(alive);
        if (!amask) return;
        if (sp == 0) return;
        sp -= W;
        cur = PT_UNIFORM_U32(wstack[sp]);
        if (STATS) in = (unsigned long long)PT_UNIFORM_U32(wstack[sp + 1]) | ((unsigned long long)PT_UNIFORM_U32(wstack[sp + 2]) << 32);
    }
}

// The frame's occluder table (pt_render_simple_kernel): per (8x8 tile, light) the node that last blocked a shadow ray of the tile
// toward the light, as node + 1 (0: none yet). `entry` = the wavefront's own entry, `back` = how many words before it the fallback
// entry lies (the tile above; 0: none), `light` = the light's index (the -DPT_OCCLUDER_STATS counts). entry == nullptr: no table.
struct PtOccRef {
    uint32_t* entry;
    uint32_t back, light;
};

// What the caller has read of the table already (the certain-shadow test in front of a light's set-up, pt_render_simple_kernel): `loaded` != 0: the two entries
// (`own`, `up`). `certain` (the -DPT_OCCLUDER_STATS=2 counts only): bit 0 (and 1) every shaded lane is certain by the candidate's ball, bit 2 the dark-light guard lets every shaded lane through.
struct PtOccHint {
    uint32_t loaded, own, up, certain;
};

// Shadow rays (any = true) test the tile's last occluder for their light first: where it blocks every lane, the walk is skipped.
// Exact by construction: a shadow ray only asks whether ANY node is hit in [EPSILON, INF) - an OR over nodes, whatever their order -
// and the cached test is the walk's own leaf test (same function, same range - `best` is still empty -, same local ray, the same
// wave-wide identity_ok). Lanes it does not block walk as before; the walk may test that node again for them, which changes nothing.
// -DPT_OCCLUDER_STATS makes the counting build count, per light, what the test would have saved (diag[], see below) without changing the walk.
// (occ.entry != nullptr; STATS only with -DPT_OCCLUDER_STATS - pt_trace_packet sees to both.)
template <bool STATS, bool HIER>
PT_HD void pt_trace_packet_occ(const PtSceneView& sc, const PtRay& ray, bool has_ray, PtHit& best, uint32_t* wstack, int wwords,
                               unsigned int* overflow, PtCounters* cnt, PtOccRef occ, PtOccHint hint) {
    constexpr bool any = true;
#if defined(__HIP_DEVICE_COMPILE__)
#ifdef PT_OCCLUDER_STATS
    constexpr bool COUNT_OCC = STATS;
#else
    constexpr bool COUNT_OCC = false;
#endif
    uint32_t* const entry = (uint32_t*)pt_uniform_ptr(occ.entry);
    const uint32_t own = hint.loaded ? hint.own : PT_UNIFORM_U32(entry[0]);
    const uint32_t up = hint.loaded ? hint.up : (occ.back ? PT_UNIFORM_U32(entry[-(long)occ.back]) : 0u);
    const uint32_t cand = own ? own : up;
    const unsigned long long rays = PT_BALLOT(has_ray);
    bool blocked = false;
    if (has_ray) { best.t = INFINITY; best.node = PT_NO_HIT; best.sub = 0; }
    if (cand != 0u && has_ray) {
        const bool identity_ok = HIER && pt_ray_identity_safe(ray, has_ray);  // (wave-uniform, as in the walk: over every lane that carries a ray)
        PtHit probe = best;
        blocked = pt_test_node_uniform<false, HIER>(sc, cand - 1u, ray, identity_ok, probe, cnt);
        if (!STATS && blocked) best = probe;
    }
    const unsigned long long blocked_mask = PT_BALLOT(blocked);
    const uint32_t first = (uint32_t)__ffsll((long long)__ballot(1)) - 1u;
    if (!STATS && blocked_mask != 0ull && blocked_mask == rays) {  // the whole wavefront in the shadow of one node: no walk
        if (own != cand && PT_LANE_ID() == first) entry[0] = cand;
        return;
    }
    if (STATS) pt_trace_packet_walk<STATS, HIER>(sc, ray, has_ray, any, best, wstack, wwords, overflow, cnt);
    else pt_trace_packet_walk<STATS, HIER>(sc, ray, has_ray, any, best, wstack, wwords, overflow, cnt, !blocked);
    // the entry: the node that blocked the lowest blocked lane; a walk in which nothing was in the way clears it (lit regions stop testing)
    const unsigned long long hit_mask = PT_BALLOT(has_ray && best.node != PT_NO_HIT);
    const uint32_t now = hit_mask ? (uint32_t)__builtin_amdgcn_readlane((int)best.node, (int)(__ffsll((long long)hit_mask) - 1)) + 1u : 0u;
    if (rays && now != own && PT_LANE_ID() == first) entry[0] = now;
    if (COUNT_OCC && rays && occ.light < 3u && PT_LANE_ID() == first) {
        // diag[2 l]: walks toward light l (low half), of them with a lane in the shadow (high half); diag[2 l + 1]: walks with EVERY lane in
        // the shadow (low), of them those the candidate alone would have ended (high); diag[6]: walks with a candidate (low; high: from the
        // own tile), diag[7]: walks in which the candidate blocked a lane (low)
        cnt->diag[2 * occ.light] += 1ull | (hit_mask ? 1ull << 32 : 0ull);
        if (hit_mask == rays) cnt->diag[2 * occ.light + 1] += 1ull | (blocked_mask == rays ? 1ull << 32 : 0ull);
#if PT_OCCLUDER_STATS + 0 == 2  // diag[6]: per light (21 bits each) the walks the candidate alone ends in which its ball settles every lane; diag[7]: the fully blocked walks the dark-light
        // guard (pt_dark_lane, hint.certain bit 2) settles. A walk it would settle in which some lane is NOT blocked would be a wrong skip: counted in kd_plane_miss, which no
        // walk of this semantics touches, and must stay 0 (profiles/occluder_stats.py checks it).
        if (hit_mask == rays && blocked_mask == rays && (hint.certain & 1u)) cnt->diag[6] += 1ull << (21 * occ.light);
        if (hint.certain & 4u) {
            if (hit_mask == rays) cnt->diag[7] += 1ull << (21 * occ.light);
            else cnt->kd_plane_miss++;
        }
#else
        if (cand) cnt->diag[6] += 1ull | (own ? 1ull << 32 : 0ull);
        if (blocked_mask) cnt->diag[7]++;
#endif
    }
#else
    pt_trace_packet_walk<STATS, HIER>(sc, ray, has_ray, any, best, wstack, wwords, overflow, cnt);
#endif
}

// The mesh-free walks' entry: shadow rays of a launch with an occluder table go through the table's test (pt_trace_packet_occ). The counting build walks as before
// (its node counts are compared with the oracle's) unless -DPT_OCCLUDER_STATS.
// EYE: primary rays (nearest hit, no table entry) whose walk reads the launch's eye table (pt_trace_packet_walk).
template <bool STATS, bool HIER, bool EYE = false>
PT_HD void pt_trace_packet(const PtSceneView& sc, const PtRay& ray, bool has_ray, bool any, PtHit& best, uint32_t* wstack, int wwords,
                           unsigned int* overflow, PtCounters* cnt, PtOccRef occ = PtOccRef{nullptr, 0u, 0u}, const double* eye_tab = nullptr) {
    if (EYE) {
        pt_trace_packet_walk<STATS, HIER, EYE>(sc, ray, has_ray, false, best, wstack, wwords, overflow, cnt, true, eye_tab);
        return;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#ifdef PT_OCCLUDER_STATS
    constexpr bool COUNT_OCC = STATS;
#else
    constexpr bool COUNT_OCC = false;
#endif
    if ((STATS && !COUNT_OCC) || !any || occ.entry == nullptr) {
        pt_trace_packet_walk<STATS, HIER>(sc, ray, has_ray, any, best, wstack, wwords, overflow, cnt);
        return;
    }
    pt_trace_packet_occ<STATS, HIER>(sc, ray, has_ray, best, wstack, wwords, overflow, cnt, occ, PtOccHint{0u, 0u, 0u, 0u});
#else
    pt_trace_packet_walk<STATS, HIER>(sc, ray, has_ray, any, best, wstack, wwords, overflow, cnt);
#endif
}

// A wave-uniform pointer pinned to a scalar register pair (see pt_args_again: what is read through the re-read argument block would
// otherwise be fetched again - one more dependent scalar load - in front of every use inside a loop).
PT_HD const void* pt_pin_ptr(const void* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long a = (unsigned long long)pt_uniform_ptr(p);
    asm volatile("" : "+s"(a));
    return (const void*)a;
#else
    return p;
#endif
}
// The walk of ONE mesh instance's triangle tree (round 5), compiled once per octant of the participating lanes' rays: descents, triangle leaves and the
// pops between them stay inside the specialised code until the instance's part of the stack is used up (`sp` back at its value on entry - no marker entry, no
// marker test per pop, no re-dispatch on the octant per descent). Returns 0: instance finished, 1: stack overflow / watchdog, 2: no lane wants candidates any more.
template <bool STATS, bool HIER, int OCT>
PT_HD int pt_walk_instance(const PtSceneView& sc, uint32_t inst, uint32_t root, const PtRay& local, const PtRayPk& q, bool part, bool any, bool& alive, PtHit& best, float& tm,
                           uint32_t* wstack, int& sp, int words, uint32_t& pops, PtCounters* cnt) {
    const int sp0 = sp;
    uint32_t cur = root;
    unsigned long long pmask = PT_BALLOT(alive && part);
    // (the tree's base address pinned to a scalar register pair: read through the re-read argument block it is a value the compiler may fetch again wherever it is
    // short of registers - and it did, in front of every node fetch of every step: one more dependent round trip through the scalar cache per step)
    const PtBvhNode* const bvh = static_cast<const PtBvhNode*>(pt_pin_ptr(sc.bvh));
    const double* const tri_leaf = static_cast<const double*>(pt_pin_ptr(sc.tri_leaf));
    for (;;) {
        if (!(cur & PT_REF_LEAF)) pt_descend_mesh<STATS, OCT>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt);
        if (cur == PT_REF_EMPTY) return 1;
        if (cur != PT_REF_POP) {
            const uint32_t first = (cur & ~PT_REF_LEAF) >> 3, count = (cur & 7u) + 1u;
            PT_WAVE_COUNT(5);
            if (STATS && alive && part) cnt->n_leaf++;
            PT_CYC_BEGIN();
            for (uint32_t i = 0; i < count; i++) {
                pt_u32x16 a;
                uint32_t b0, b1;
                const uint32_t tri = pt_load_leaf_triangle_at(tri_leaf, first + i, a, b0, b1);
                double tv[9];
#pragma unroll
                for (int k = 0; k < 8; k++) tv[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
                tv[8] = pt_f64_of(b0, b1);
                if (alive && part) {
                    double tt, beta, gamma;
                    if (STATS) cnt->n_tri++;
                    if (PT_TRI_HIT(tv, local, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, inst, tri), &tt, &beta, &gamma)) {
                        best.t = tt; best.node = inst; best.sub = tri;
                        tm = pt_tmax32(tt);
                        if (any) alive = false;
                    }
                }
            }
            PT_CYC_END(5);
            if (!PT_BALLOT(alive)) return 2;
            pmask = PT_BALLOT(alive && part);
        }
        if (sp == sp0) return 0;
        if (++pops > PT_WALK_POPS_MAX) return 1;
        sp--;
        cur = PT_UNIFORM_U32(wstack[sp]);
    }
}

// The same for scenes WITH mesh instances (PT_MODE_FLAT, hits spawn no rays): the scene tree and every mesh's triangle tree are
// walked once per wavefront. Entering a mesh instance is wave-uniform too: every lane brings its ray into the instance's space
// with the one inverse transform (scalar operands), the lanes whose rays pass the mesh's exact box test (mesh.rs:146-155) take
// part in its tree (pt_walk_instance), and the scene tree continues where the instance's part of the stack is used up. Triangle records (nine doubles) arrive through
// the scalar cache like nodes. Two-child nodes throughout (the array the four-child form is made from).
// KDMESH: KDMesh instances keep the reference's own triangle k-d tree (quirk Q3), which every lane walks by itself with its own
// range bookkeeping (pt_kdmesh_hit) on `lane_stk`, a per-lane stack beside the wavefront's. HIER: the hierarchical semantics
// (every SceneNode's own inverse on the way down, ties by depth-first rank).
template <bool STATS, bool KDMESH, bool HIER, class LaneStack>
PT_HD void pt_trace_packet_mesh(const PtSceneView& sc, const PtRay& ray, bool has_ray, bool any, PtHit& best, uint32_t* wstack, int wwords,
                                const LaneStack& lane_stk, unsigned int* overflow, PtCounters* cnt) {
    if (has_ray) { best.t = PT_WALK_ENTRY_T(best); best.node = PT_NO_HIT; best.sub = 0; }
    if (sc.n_nodes == 0 || sc.tlas_root == PT_REF_EMPTY) return;
    // (Since round 5 a mesh instance's tree is walked by pt_walk_instance and nothing pushes PT_REF_MARKER here: `inst` stays PT_NO_HIT, `part` has_ray, `local` the ray,
    // `oct` PT_OCT_MIXED, `entered` false, and the leaf's triangle branch and the marker's pop below are never taken. They are what is left of the walk that kept an
    // instance's tree on this stack, and they stay for now: this function's machine code changes with any one of them taken out - the loop over a leaf's nodes without
    // `entered` alone - and every kernel of the modes with mesh instances was tuned and measured with the code as it is.)
    bool alive = has_ray;     // the lane still wants candidates
    bool part = has_ray;      // ... and takes part in the tree being walked (inside a mesh: its ray passed the mesh's box test)
    unsigned long long pmask = PT_BALLOT(alive && part);  // the lanes the slab test's results count for, as a wave-uniform mask
    PtRay local = ray;        // the ray in the space of the tree being walked
    PtRayPk q = pt_raypk(ray);
    int oct = PT_OCT_MIXED;   // wave-uniform: the octant the participating lanes' rays share inside the mesh instance being walked, if they do (sc.mesh_oct)
    const bool identity_ok = HIER && pt_ray_identity_safe(ray, has_ray);  // (wave-uniform) levels of a path that are the identity may be skipped
    float tm = PT_WALK_ENTRY_TM(best);      // best.t as the f32 bound of the slab test (t means the same in every space, ray.rs:130-135)
    uint32_t inst = PT_NO_HIT;  // wave-uniform: flat node of the mesh instance being walked
    uint32_t cur = PT_UNIFORM_U32(sc.tlas_root);
    int sp = 0;
    auto slot = [&](int k) -> uint32_t& { return wstack[k]; };
    const int words = wwords < sc.stack_cap ? wwords : sc.stack_cap;
    uint32_t pops = 0;  // (watchdog: pending subtrees taken by this walk; one that takes more than any tree has nodes ends like a stack overflow)
    // (the scene-level steps' base address: pinned in the instantiations with KDMesh trees, whose walks are mostly scene-level steps - the dielectric workload +1.0 %, its hierarchical form +1.6 %; left to
    // the compiler in the others, where the pair of registers costs the mirror scene 0.4 % - c55)
    const PtBvhNode* const bvh = KDMESH ? static_cast<const PtBvhNode*>(pt_pin_ptr(sc.bvh)) : sc.bvh;
    const uint32_t* const info_base = sc.info;
    const double* const inv_base = sc.inv;
    const PtMeshInfo* const meshes_base = sc.meshes;
    auto overflowed = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        if (overflow) atomicOr(overflow, pops > PT_WALK_POPS_MAX ? 4u : 1u);  // 4: the watchdog
#endif
        if (STATS) cnt->stack_overflow++;
        if (has_ray) best.node = PT_NO_HIT;
    };
    for (;;) {
        // down to the next leaf (pt_descend_mesh): a leaf reference, PT_REF_POP when neither child is reached, PT_REF_EMPTY when the
        // stack overflowed. Always the per-lane form of the slab test: the walks of these scenes are short (5.7 tree steps per ray on
        // macho-cows, 8.6 on the mirror scene) and the octant bookkeeping per ray and per mesh instance cost more than the eight
        // instructions per step it saves (cows -6 %, mirror -3 %; big-scene, mesh-free, +4 %: profiles/r03/notes.md).
        // Round 4 (sc.mesh_oct): INSIDE a mesh instance whose lanes' rays share their direction signs the sorted form runs (`oct`, worked out once per
        // instance entered; the scene-level steps keep the per-lane form): 37 steps per ray on the 1.25 M-triangle soup +6 %, the short walks no longer lose.
        if (!(cur & PT_REF_LEAF)) {
            switch (STATS ? PT_OCT_MIXED : oct) {
            case 0: pt_descend_mesh<STATS, 0>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 1: pt_descend_mesh<STATS, 1>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 2: pt_descend_mesh<STATS, 2>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 3: pt_descend_mesh<STATS, 3>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 4: pt_descend_mesh<STATS, 4>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 5: pt_descend_mesh<STATS, 5>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 6: pt_descend_mesh<STATS, 6>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            case 7: pt_descend_mesh<STATS, 7>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            default: pt_descend_mesh<STATS, PT_OCT_MIXED>(bvh, q, tm, pmask, alive && part, cur, sp, wstack, words, cnt); break;
            }
        }
        if (cur == PT_REF_EMPTY) { overflowed(); return; }
        const bool popped = cur == PT_REF_POP;
        if (!popped) {
            const uint32_t first = (cur & ~PT_REF_LEAF) >> 3, count = (cur & 7u) + 1u;
            PT_WAVE_COUNT(5);
            if (STATS && alive && part) cnt->n_leaf++;
            if (inst != PT_NO_HIT) {  // triangles of the mesh being walked
                PT_CYC_BEGIN();
                for (uint32_t i = 0; i < count; i++) {
                    pt_u32x16 a;
                    uint32_t b0, b1;
                    const uint32_t tri = pt_load_leaf_triangle(sc, first + i, a, b0, b1);
                    double tv[9];
#pragma unroll
                    for (int k = 0; k < 8; k++) tv[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
                    tv[8] = pt_f64_of(b0, b1);
                    if (alive && part) {
                        double tt, beta, gamma;
                        if (STATS) cnt->n_tri++;
                        if (PT_TRI_HIT(tv, local, PT_EPSILON, pt_cand_end_in<HIER>(sc, best, inst, tri), &tt, &beta, &gamma)) {
                            best.t = tt; best.node = inst; best.sub = tri;
                            tm = pt_tmax32(tt);
                            if (any) alive = false;
                        }
                    }
                }
                PT_CYC_END(5);
            } else {
                bool entered = false;
                for (uint32_t i = 0; i < count && !entered; i++) {
                    const uint32_t node = sc.tlas_direct ? first : PT_UNIFORM_U32(sc.bvh_items[first + i]);
                    // (fetches that depend on each other cost a round trip through the scalar cache each - a mesh instance is entered with three: the
                    // node's {type, data, ..}, its inverse, the mesh record's {box inverse, roots} - not with one per field: round 4, c47)
                    const pt_u32x4 info4 = pt_sload4(info_base + 4 * (size_t)node);
                    const uint32_t type = info4[0];
                    if (type == PT_MESH || type == PT_KDMESH) {
                        const uint32_t data = info4[1];
                        const PtMeshInfo* mi = meshes_base + data;
                        PtRay lr;
                        if (HIER) {
                            lr = pt_node_local_ray_uniform(sc, node, ray, identity_ok);
                        } else {
                            double m[12];
                            pt_sload_mat12(inv_base + 12 * (size_t)node, m);
                            lr = pt_ray_to_local(m, ray);
                        }
                        if (STATS && alive) cnt->n_analytic++;
                        double bi[12];
                        pt_u32x4 head;  // {tri_first, tri_count, blas_root, kd_root}
                        pt_sload_mat12_x4(mi->bbox_inv, bi, head);
                        if (KDMESH && type == PT_KDMESH && (int32_t)head[3] >= 0) {  // the reference's own triangle tree (quirk Q3)
                            if (alive) {
                                double t; uint32_t tri = 0;
                                if (PT_WALK_KDMESH_HIT(STATS, HIER, sc, *mi, lr, best, node, lane_stk, &t, &tri, cnt)) {
                                    best.t = t; best.node = node; best.sub = tri;
                                    tm = pt_tmax32(t);
                                    if (any) alive = false;
                                }
                            }
                            continue;
                        }
                        // mesh.rs:146-155: box test, then the triangles (also a KDMesh without a tree of its own: PORTRAYER_KDMESH_AS_MESH)
                        const uint32_t root = head[2];
                        if (STATS && alive) cnt->n_bbox++;
                        if (root == PT_REF_EMPTY) continue;
                        const bool inside = alive && pt_bbox_test_hit(bi, lr, PT_EPSILON, PT_WALK_MESH_BOX_END(HIER, sc, best, node));
                        const unsigned long long inside_mask = PT_BALLOT(inside);
                        if (!inside_mask) continue;
                        {   // the instance's tree, in the code of its octant (pt_walk_instance); the scene-level walk goes on with this leaf's next node afterwards
                            int io = PT_OCT_MIXED;
                            const PtRayPk qi = (sc.mesh_oct && !STATS) ? pt_raypk(lr, inside, &io) : pt_raypk(lr);
                            int rc;
                            switch (io) {
                            case 0: rc = pt_walk_instance<STATS, HIER, 0>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 1: rc = pt_walk_instance<STATS, HIER, 1>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 2: rc = pt_walk_instance<STATS, HIER, 2>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 3: rc = pt_walk_instance<STATS, HIER, 3>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 4: rc = pt_walk_instance<STATS, HIER, 4>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 5: rc = pt_walk_instance<STATS, HIER, 5>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 6: rc = pt_walk_instance<STATS, HIER, 6>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            case 7: rc = pt_walk_instance<STATS, HIER, 7>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            default: rc = pt_walk_instance<STATS, HIER, PT_OCT_MIXED>(sc, node, root, lr, qi, inside, any, alive, best, tm, wstack, sp, words, pops, cnt); break;
                            }
                            if (rc == 1) { overflowed(); return; }
                            if (rc == 2) return;
                        }
                    } else if (alive) {
                        if (pt_test_node_uniform<STATS, HIER>(sc, node, ray, identity_ok, best, cnt)) {
                            tm = pt_tmax32(best.t);
                            if (any) alive = false;
                        }
                    }
                }
                if (entered) { pmask = PT_BALLOT(alive && part); continue; }
            }
            if (!PT_BALLOT(alive)) return;
            pmask = PT_BALLOT(alive && part);
        }
        // the next pending subtree; a marker ends the walk of a mesh instance
        for (;;) {
            if (sp == 0) return;
            if (++pops > PT_WALK_POPS_MAX) { overflowed(); return; }
            sp--;
            cur = PT_UNIFORM_U32(slot(sp));
            if (cur != PT_REF_MARKER) break;
            inst = PT_NO_HIT; local = ray; part = has_ray;
            q = pt_raypk(ray); oct = PT_OCT_MIXED;
            pmask = PT_BALLOT(alive && part);
        }
    }
}
