// Part of pt_trace.h, included after pt_walk_wave.h: lane predicates as masks, PtKdSav and the one walk per wavefront of the k-d semantics (pt_trace_packet_kd).
#pragma once

// ------------------------------------------------------------------------------------------------
// ONE walk per wavefront in the reference's k-d tree semantics (round 4; kdtree/node.rs:66-203).
//
// What the reference computes for a ray: the leaves on its path in front-to-back order, each with the range [start, end) the planes
// of the straddled splits above it leave (node.rs:139-186), and the hit of the FIRST leaf that reports one (node.rs:153-157) - a
// leaf's hit being the nearest in ITS range with the leaf's list order breaking exact ties (ray.rs:87-99). The ranges of a ray's
// leaves are disjoint half-open intervals in path order, so "the first leaf with a hit" is "the leaf hit with the smallest t", and a
// leaf's hit depends on nothing but the leaf and its range: the leaves of a ray may be visited in ANY order as long as each is
// tested with the range the reference would give it. (Cone / Cylinder results depend on the range start - quirk Q1, cone.rs:64-76 -,
// which is why the ranges must be the reference's own numbers: every plane parameter below is computed by the reference's
// expression, (plane - o) / d in f64, from the reference's side tests.)
//
// That makes the walk a change of schedule like pt_trace_packet: the NODE and the stack are wave-uniform (a node = 64 bytes through
// the scalar cache, planes and cull boxes as scalar operands), every lane carries its own (start, end), and a split sends each lane's
// range where the reference sends it:
//   * both ends of the lane's classification segment on one side (node.rs:128-137): that child, range unchanged;
//   * straddling (node.rs:139-186): its near side gets [start, plane_t), its far side [plane_t, end);
//   * plane_t outside the range (node.rs:146-147 panics): neither (counted as kd_plane_miss).
// The wavefront enters the child most of its lanes call near first; the other waits on the wavefront's stack. Lanes skip nodes that
// cannot improve their result (start > best.t: every hit below has t >= start).
//
// Where a lane's range lives: (start, end) of the CURRENT node in registers; entering a child replaces at most ONE bound by plane_t,
// and the bound it replaces goes to the lane's slot of that LEVEL (`sav`: one f64 per lane and tree level - LDS for the deepest
// levels, which the walk toggles between, HBM for the top ones). Two bits per level and lane (`codes`) say which bound the slot
// holds: 2 = the END to put back, 3 = the START to put back, 1 = the lane waits for the second child with its range unchanged,
// 0 = nothing. Popping the stack entry (second child of level L) puts back the bounds of the finished levels below L one by one,
// then turns the first child's range into the second's: for a lane with [start, plane_t) the second child gets [plane_t, saved end),
// and the slot now keeps `start` for the way back up; mirror-inverted for a lane that went far side first.
// Nothing here is kept per stack ENTRY and lane (that would be 16 bytes x 64 lanes x depth of LDS per wavefront).
// ------------------------------------------------------------------------------------------------
// ---- Lane predicates as 64-bit MASKS in scalar registers. A compare writes its result there anyway (v_cmp ... -> an SGPR pair), mask
// logic is scalar arithmetic, "any lane?" is a scalar compare with zero, and a select reads the mask back as its condition
// (inverse ballot = a plain copy). Written with `bool`s and __ballot() the compiler materialises every predicate that is not itself a
// compare as 0 / 1 in a vector register and compares that again - two vector instructions per ballot, about sixteen per tree step.
// (The masks cover the lanes that are ACTIVE where the compare executes: use them in wave-uniform control flow only.)
typedef unsigned long long pt_mask;
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_MASK_ALL (~0ull)
#define PT_F64_LT(a, b) __builtin_amdgcn_fcmp((double)(a), (double)(b), 4)   // ordered <
#define PT_F64_LE(a, b) __builtin_amdgcn_fcmp((double)(a), (double)(b), 5)   // ordered <=
#define PT_F64_GE(a, b) __builtin_amdgcn_fcmp((double)(a), (double)(b), 3)   // ordered >=
#define PT_F32_GT(a, b) __builtin_amdgcn_fcmpf((float)(a), (float)(b), 2)    // ordered >
#define PT_U32_EQ(a, b) __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 32)
#define PT_U32_GE(a, b) __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 35)
#define PT_U32_LE(a, b) __builtin_amdgcn_uicmp((unsigned)(a), (unsigned)(b), 37)
#define PT_LANES(m) __builtin_amdgcn_inverse_ballot_w64(m)
#define PT_POPC(m) __builtin_popcountll(m)
#else
#define PT_MASK_ALL 1ull
#define PT_F64_LT(a, b) (((double)(a) < (double)(b)) ? 1ull : 0ull)
#define PT_F64_LE(a, b) (((double)(a) <= (double)(b)) ? 1ull : 0ull)
#define PT_F64_GE(a, b) (((double)(a) >= (double)(b)) ? 1ull : 0ull)
#define PT_F32_GT(a, b) (((float)(a) > (float)(b)) ? 1ull : 0ull)
#define PT_U32_EQ(a, b) (((unsigned)(a) == (unsigned)(b)) ? 1ull : 0ull)
#define PT_U32_GE(a, b) (((unsigned)(a) >= (unsigned)(b)) ? 1ull : 0ull)
#define PT_U32_LE(a, b) (((unsigned)(a) <= (unsigned)(b)) ? 1ull : 0ull)
#define PT_LANES(m) ((m) != 0ull)
#define PT_POPC(m) ((int)((m) & 1ull))
#endif
#define PT_MNOT(m) (~(m) & PT_MASK_ALL)
// pt_in_range as a mask: start <= t && t < end (false for NaN)
PT_HD pt_mask pt_in_range_m(double start, double end, double t) { return PT_F64_LE(start, t) & PT_F64_LT(t, end); }
// pt_slab_seg_pk as a mask: the lanes whose segment [tmin, tmax] reaches the box
PT_HD pt_mask pt_slab_seg_pk_m(const float* lo, const float* hi, const PtRayPk& q, float tmin, float tmax) {
    const float ax = __builtin_fmaf(lo[0], q.a[0].x, q.a[0].y), bx = __builtin_fmaf(hi[0], q.b[0].x, q.b[0].y);
    const float ay = __builtin_fmaf(lo[1], q.a[1].x, q.a[1].y), by = __builtin_fmaf(hi[1], q.b[1].x, q.b[1].y);
    const float az = __builtin_fmaf(lo[2], q.a[2].x, q.a[2].y), bz = __builtin_fmaf(hi[2], q.b[2].x, q.b[2].y);
    const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax));
    return PT_MNOT(PT_F32_GT(tn, tf));
}
PT_HD pt_mask pt_div_exp_ok_m(double x) {
    union { double d; uint32_t u[2]; } c; c.d = x;
    return PT_U32_LE(((c.u[1] >> 20) & 0x7FFu) - 640u, 767u);
}

// "does any lane ...": the ballot as a 64-bit scalar compared with zero on the SCALAR unit. Written as `if (__ballot(x))` the compiler
// materialises the predicate as 0 / 1 in a vector register and compares that again (two vector instructions per wave-uniform branch).
PT_HD bool pt_any(bool b) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long m = __ballot(b);
    asm volatile("" : "+s"(m));
    return m != 0ull;
#else
    return b;
#endif
}
// 8 dwords at base + byte offset (32 bits): one scalar load, no 64-bit address arithmetic
PT_HD pt_u32x8 pt_sload8_off(const void* base, uint32_t byte_off) {
    pt_u32x8 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx8 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "s"(byte_off) : "memory");
#else
    v = *reinterpret_cast<const pt_u32x8*>(static_cast<const char*>(base) + byte_off);
#endif
    return v;
}

PT_HD pt_u32x16 pt_sload16_off(const void* base, uint32_t byte_off) {
    pt_u32x16 v;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "s"(byte_off) : "memory");
#else
    v = *reinterpret_cast<const pt_u32x16*>(static_cast<const char*>(base) + byte_off);
#endif
    return v;
}

// (pt_rcp_refined / pt_div_exp_ok / pt_div_fast - the short f64 division by a repeated denominator - live in pt_math.h)

// The lanes' replaced range bounds per tree level (see pt_trace_packet_kd). Round 5: only the DEEP levels keep a slot (in LDS); a bound replaced at one of
// the `top_levels` levels nearest the root is not stored at all - it is recomputed when the walk comes back to that level:
//   at any node, a lane's `end` is the plane parameter of the DEEPEST level above it whose code says "straddled, now in the near child" (code 2), or
//   infinity; its `start` is that of the deepest level with code 3 ("straddled, now in the far child"), or epsilon - the codes (two bits per level, in a
//   register) and the planes of the current path determine the range completely. The path is the same for every lane of the wavefront, so the planes of
//   its top levels sit in a small table in the wavefront's LDS (`path`: plane lo, plane hi, axis per level), and a plane parameter is recomputed with the very
//   expression that produced it, (plane - o) / d: the same bits.
// (Round 4 stored the top levels' bounds in the lanes' HBM columns: 16 bytes per lane, level and ray written and read back - 30 GB per big-scene frame.)
struct PtKdSav {
    uint32_t* lds;        // the wavefront's rows for saved bounds: level k >= top_levels in slot k - top_levels; slot j, half h of lane l at lds[(2 j + h) * 64 + l]
    int top_levels;       // levels [0, top_levels) keep no slot: recomputed from `path`
    uint32_t* path;       // the wavefront's table of the current path's top levels: path[3 k] / [3 k + 1] the plane (f64 halves), path[3 k + 2] the axis
};
PT_HD void pt_kd_sav_store(const PtKdSav& s, int level, double v) {  // `level` is wave-uniform and >= s.top_levels
    union { double d; uint32_t u[2]; } c; c.d = v;
    uint32_t* p = s.lds + (size_t)(2 * (level - s.top_levels)) * 64 + PT_LANE_ID();
    p[0] = c.u[0]; p[64] = c.u[1];
}
PT_HD double pt_kd_sav_load(const PtKdSav& s, int level) {
    union { double d; uint32_t u[2]; } c;
    const uint32_t* p = s.lds + (size_t)(2 * (level - s.top_levels)) * 64 + PT_LANE_ID();
    c.u[0] = p[0]; c.u[1] = p[64];
    return c.d;
}
#define PT_KD_WALK_STEPS_MAX (1u << 26)  // more nodes than a k-d tree of 2^26 nodes (the limit of the 32-bit byte offsets) has
#define PT_KD_WAVE_LEVELS 32  // two bits per level in a 64-bit word per lane. pt_scene_upload REFUSES deeper trees (PT_ERR_SCENE; include/portrayer_hip.h says so):
                              // the render kernels have no other k-d walk (the per-lane PtKdWalker serves pt_test_cast_rays only)

// Mesh::ray_hit below a k-d leaf (mesh.rs:146-167) for the lanes in `part`: the instance's triangle tree walked once per wavefront
// like pt_trace_packet_mesh does, every triangle tested over [start, end of the lane's leaf fold) - nearest triangle, lowest index on
// exact ties (pt_cand_end), which is what the reference's fold over ALL triangles with a shrinking range gives. `wstack`: free words
// of the wavefront's stack. Returns false when they ran out.
template <bool STATS, int OCT>
PT_HD bool pt_packet_mesh_below_kd_oct(const PtSceneView& sc, uint32_t inst, uint32_t root, const PtRay& local, const PtRayPk& q, bool part, double start, bool any, PtHit& lb, bool& found,
                                       uint32_t* wstack, int words, PtCounters* cnt) {
    float tm = pt_tmax32(lb.t);
    // the lane's range starts at `start` (the k-d leaf's): boxes that end before it hold no hit of this leaf - a mesh that spans several k-d leaves
    // is walked once per leaf, each time only where the leaf's range reaches (round 4). Rounded down like the k-d walk's own segment culls.
    float t0 = (float)start;
    t0 = t0 - fabsf(t0) * 2.4e-7f;
    unsigned long long pmask = PT_BALLOT(part);
    uint32_t cur = root;
    int sp = 0;
    uint32_t steps = 0;  // (watchdog, as in pt_trace_packet_kd: leaves visited)
    // (not pinned as in pt_walk_instance: this function runs once per k-d leaf an instance spans, and pinned for the mirror scene's small meshes the k-d frame
    // was 7 % slower: 41.1 -> 44.3 ms, c62)
    const PtBvhNode* const bvh = sc.bvh;
    const double* const tri_leaf = sc.tri_leaf;
    for (;;) {
        if (!(cur & PT_REF_LEAF)) pt_descend_mesh<STATS, OCT, true>(bvh, q, tm, pmask, part, cur, sp, wstack, words, cnt, t0);
        steps++;
        if (cur == PT_REF_EMPTY || steps > PT_KD_WALK_STEPS_MAX) return false;
        if (cur != PT_REF_POP) {
            const uint32_t first = (cur & ~PT_REF_LEAF) >> 3, count = (cur & 7u) + 1u;
            if (STATS && part) cnt->n_leaf++;
            for (uint32_t i = 0; i < count; i++) {
                pt_u32x16 a;
                uint32_t b0, b1;
                const uint32_t tri = pt_load_leaf_triangle_at(tri_leaf, first + i, a, b0, b1);
                double tv[9];
#pragma unroll
                for (int k = 0; k < 8; k++) tv[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
                tv[8] = pt_f64_of(b0, b1);
                if (part) {
                    double tt, beta, gamma;
                    if (STATS) cnt->n_tri++;
                    if (PT_TRI_HIT(tv, local, start, pt_cand_end(lb, inst, tri), &tt, &beta, &gamma)) {
                        lb.t = tt; lb.node = inst; lb.sub = tri;
                        found = true;
                        tm = pt_tmax32(tt);
                        if (any) part = false;  // a shadow ray only asks whether anything is in the way (material.rs:174-179)
                    }
                }
            }
            pmask = PT_BALLOT(part);
            if (!pmask) return true;
        }
        if (sp == 0) return true;
        sp--;
        cur = PT_UNIFORM_U32(wstack[sp]);
    }
}

template <bool STATS>
PT_HD bool pt_packet_mesh_below_kd(const PtSceneView& sc, uint32_t inst, uint32_t root, uint32_t tri_count, const PtRay& local, bool part, double start, bool any, PtHit& lb, bool& found,
                                   uint32_t* wstack, int words, PtCounters* cnt) {
    // ONE instantiation, the per-lane form. Octant instantiations like pt_walk_instance's, taken by instances of >= 65,536 triangles, made the 1.25 M-triangle soup's k-d frame
    // 8 - 10 % faster - and, by being in the kernel at all, the mirror scene's 6.4 % and macho-cows' 1.7 % slower (registers, code size): c64. The reference's own scenes decide.
    // (Taken by every instance they lost more: the soup +5.4 %, the mirror scene's and macho-cows' few-thousand-triangle meshes, walked once per k-d leaf they span, -6.6 % / -3.7 % - c49.)
    (void)tri_count;
    return pt_packet_mesh_below_kd_oct<STATS, PT_OCT_MIXED>(sc, inst, root, local, pt_raypk(local), part, start, any, lb, found, wstack, words, cnt);
}

// One split of the k-d walk for the lanes in `mine` (node.rs:112-186): which side the ends of the lane's classification segment are on
// (s, e: Front), who crosses the plane, where (plane_t = (plane - o) / d, node.rs:90-109) and who straddles it inside the range.
PT_HD void pt_kd_split_eval(double o, double d, double y, pt_mask d_ok, double plane, double t_min, double t_max, double start, double end, pt_mask mine,
                            pt_mask* s_out, pt_mask* e_out, pt_mask* cross_out, pt_mask* strad_out, double* plane_t_out) {
    const pt_mask s = PT_F64_GE((o + d * t_min) - plane, 0.0);  // infinite_plane.rs:27-35: Front
    const pt_mask e = PT_F64_GE((o + d * t_max) - plane, 0.0);
    const pt_mask cross = mine & (s ^ e);
    double plane_t = 0.0;
    pt_mask strad = 0ull;
    if (cross) {
        const double n = plane - o;
        const pt_mask fast = d_ok & pt_div_exp_ok_m(n);
        if (cross & PT_MNOT(fast)) plane_t = n / d;   // some crossing lane's operands are outside the short division's window
        else plane_t = pt_div_fast(n, d, y);
        strad = cross & pt_in_range_m(start, end, plane_t);
    }
    *s_out = s; *e_out = e; *cross_out = cross; *strad_out = strad; *plane_t_out = plane_t;
}

// plane_t = (plane - o) / d of pt_kd_split_eval for the lanes in `who`, computed again (a pop at a top level: PtKdSav): the short division where every such
// lane's operands are inside its window, else the hardware's - either way the quotient `/` gives, so the very bits the split produced.
PT_HD double pt_kd_plane_t(double o, double d, double y, pt_mask d_ok, double plane, pt_mask who) {
    const double n = plane - o;
    const pt_mask fast = d_ok & pt_div_exp_ok_m(n);
    if (who & PT_MNOT(fast)) return n / d;
    return pt_div_fast(n, d, y);
}

// wstack: the wavefront's own stack (linear, `wwords` words); sav: the lanes' saved bounds per level; lane_stk: the lanes' own stacks
// (KDMESH only: KDMesh instances keep the reference's triangle k-d tree, which every lane walks by itself, pt_kdmesh_hit).
template <bool STATS, bool MESH, bool KDMESH, class LaneStack>
PT_HD void pt_trace_packet_kd(const PtSceneView& sc, const PtRay& ray_in, bool has_ray, bool any, PtHit& best, uint32_t* wstack, int wwords, const PtKdSav& sav,
                              const LaneStack& lane_stk, unsigned int* overflow, PtCounters* cnt) {
    // (a copy: picking a component by the split's axis from a ray behind a REFERENCE becomes a load from a selected address, and the
    // caller's ray then lives in scratch memory and is indexed there at every split)
    const PtRay ray = ray_in;
    if (has_ray) { best.t = INFINITY; best.node = PT_NO_HIT; best.sub = 0; }
    // lane predicates are masks in scalar registers (see PT_LANES)
    pt_mask alive = PT_BALLOT(has_ray);   // the lanes that still want candidates (a shadow ray stops at its first hit)
    pt_mask in = alive;                   // the lanes taking part in the subtree of `cur`
    const pt_mask any_m = PT_BALLOT(any);
    double start = PT_EPSILON, end = INFINITY;  // ray.rs:140; the lane's range at the current node
    uint32_t codes_lo = 0, codes_hi = 0;        // two bits per level of the current path (see above): levels 0-15 / 16-31
    const PtRayPk q = pt_raypk(ray);
    const double extent = sc.kd_extent;
    // per axis: the refined reciprocal of the direction component and whether the short division may be used with it (pt_div_fast)
    const double yx = pt_rcp_refined(ray.d.x), yy = pt_rcp_refined(ray.d.y), yz = pt_rcp_refined(ray.d.z);
    const pt_mask okx = pt_div_exp_ok_m(ray.d.x), oky = pt_div_exp_ok_m(ray.d.y), okz = pt_div_exp_ok_m(ray.d.z);
    const void* const kd_base = pt_pin_ptr(sc.kd);
    const void* const ref_base = pt_pin_ptr(sc.kd_ref);
    uint32_t cull = PT_UNIFORM_U32((sc.kd_box != nullptr ? 1u : 0u) | (sc.node_box != nullptr ? 2u : 0u));  // (PORTRAYER_KD_NO_CULL clears both)
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(cull));  // (a scalar the walk branches on: left alone the two flags were re-materialised through the vector unit - v_cndmask, v_cmp - at every node and every leaf reference)
#endif
    uint32_t cur = 0;                 // wave-uniform: node, its level, words on the stack
    int lev = 0, sp = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    // (pinned to scalar registers from the start: the constant 0 otherwise reaches the loop's phi as a copy of some VECTOR register that
    // also holds a 0, and the compiler's SGPR-copy fixing then moves the whole chain - and the scalar load's offset - to the vector side)
    asm volatile("" : "+s"(cur), "+s"(lev), "+s"(sp));
#endif
    // ONE way out of the walk (the test at the very end of the body): an early `return` from inside these loops - with the lanes' divergent
    // code of the failure path behind it - makes the compiler's unified loop exit a join of divergent branches, and every wave-uniform value
    // that passes through it (the node index, the stack pointer, the lane masks) is then taken for divergent: no scalar loads, no SALU block.
    // For the same reason the lanes' own updates below are selects, not branches.
    bool failed = false;   // wave-uniform: the wavefront's stack overflowed, or the watchdog below tripped
    uint32_t steps = 0;    // wave-uniform: nodes visited by this walk. A walk visits a node at most once; one that goes on beyond any tree this
                           // library accepts is a defect (or a corrupted stack) and fails the render (PT_ERR_TRAVERSAL) instead of hanging the GPU
    float seg0c = 0.0f, seg1c = 0.0f;
    if (!MESH) {
        seg0c = (float)start; seg1c = (float)end;
        seg0c = seg0c - fabsf(seg0c) * 2.4e-7f; seg1c = seg1c + fabsf(seg1c) * 2.4e-7f;
    }
    for (;;) {
        steps++;
        failed = failed || steps > PT_KD_WALK_STEPS_MAX;
        bool descend = false;  // wave-uniform: go on with `cur` (a child) instead of taking the next pending subtree
        // the lanes this node can still give something: taking part, and no hit yet in front of everything below (every hit
        // below has t >= start, and ranges of different leaves never share a t)
        pt_mask mine = failed ? 0ull : (alive & in & PT_MNOT(PT_F64_LT(best.t, start)));
        if (mine) {
            const pt_u32x16 v = pt_sload16_off(kd_base, cur << 6);
            PT_WAVE_COUNT(4);
            // the lane's segment [start, end), rounded outward, against the conservative f32 bounds of everything below this node:
            // a subtree the segment does not reach reports no hit, which is all the reference would find out by walking it
            // (the f32 segment is kept across nodes and converted again only where start / end change - a straddled split, a pop: +0.3 %, c70)
            float seg0 = seg0c, seg1 = seg1c;
            if (MESH) {  // (the instantiations with mesh walks below the leaves lose with the two registers held across the walk - mirror k-d -2.8 %, c71 - and convert per node)
                seg0 = (float)start; seg1 = (float)end;
                seg0 = seg0 - fabsf(seg0) * 2.4e-7f; seg1 = seg1 + fabsf(seg1) * 2.4e-7f;
            }
            if (cull & 1u) {
                const float lo[3] = {pt_f32_of(v[8]), pt_f32_of(v[9]), pt_f32_of(v[10])}, hi[3] = {pt_f32_of(v[11]), pt_f32_of(v[12]), pt_f32_of(v[13])};
                const pt_mask reach = pt_slab_seg_pk_m(lo, hi, q, seg0, seg1);
                if (STATS && PT_LANES(mine & PT_MNOT(reach))) cnt->kd_culled++;
                mine &= reach;
            }
            const int axis = (int)v[2];
            if (axis >= 0) {
                // ---- a split (node.rs:112-202), for the lanes in `mine`
                if (STATS && PT_LANES(mine)) cnt->n_inner++;
                const double plane = pt_f64_of(v[0], v[1]);
                double t_max = start + extent;                                   // node.rs:118
                t_max = PT_LANES(pt_in_range_m(start, end, t_max)) ? t_max : end - PT_EPSILON;   // node.rs:121
                const double t_min = start + PT_EPSILON;                         // node.rs:124
                // (the same arithmetic compiled once per axis, behind a scalar branch: picking o, d and the reciprocal by a run-time axis
                // cost twelve selects per split, c62)
                pt_mask s, e, cross, strad;
                double plane_t;
                if (axis == 0) pt_kd_split_eval(ray.o.x, ray.d.x, yx, okx, plane, t_min, t_max, start, end, mine, &s, &e, &cross, &strad, &plane_t);
                else if (axis == 1) pt_kd_split_eval(ray.o.y, ray.d.y, yy, oky, plane, t_min, t_max, start, end, mine, &s, &e, &cross, &strad, &plane_t);
                else pt_kd_split_eval(ray.o.z, ray.d.z, yz, okz, plane, t_min, t_max, start, end, mine, &s, &e, &cross, &strad, &plane_t);
                if (STATS && PT_LANES(cross & PT_MNOT(strad))) cnt->kd_plane_miss++;  // node.rs:146-147 / :177-178: the reference panics here; a miss for this subtree
#if defined(__HIP_DEVICE_COMPILE__)  // (the host takes every split through the general bookkeeping, below; on the device that was c62's slower side)
                // The common case settled in seven scalar instructions (the pattern of pt_descend's step): no lane's segment crosses the plane and every lane is on one
                // side - that child next, nothing waits, no range changes, code 0. `slow_`: everything else, through the general bookkeeping. ONE place assigns the node index.
                uint32_t c_first, slow_, f_;
                pt_mask t_;
                asm volatile(
                    "s_and_b64 %[t], %[mine], %[s]\n\t"
                    "s_cselect_b32 %[next], %[cf], %[cb]\n\t"
                    "s_cselect_b32 %[f], 1, 0\n\t"
                    "s_andn2_b64 %[t], %[mine], %[s]\n\t"
                    "s_cselect_b32 %[slow], %[f], 0\n\t"
                    "s_cmp_lg_u64 %[cross], 0\n\t"
                    "s_cselect_b32 %[slow], 1, %[slow]"
                    : [next] "=&s"(c_first), [slow] "=&s"(slow_), [f] "=&s"(f_), [t] "=&s"(t_)
                    : [mine] "s"(mine), [s] "s"(s), [cross] "s"(cross), [cf] "s"(v[3]), [cb] "s"(v[4])
                    : "scc");
                pt_mask in_first = mine;
                uint32_t code = 0u;
                descend = mine != 0ull && !failed;
                if (slow_) {
                    // (the general case's mask algebra in one block of scalar instructions too - c61's block, which lost when every split issued it, issued only where all
                    // of it is needed: +0.9 % against the compiler's version, c74)
                    pt_mask go_f, go_b, in_second, t0_, t1_;
                    uint32_t c_second, ff_, push_, any_, nf_, nb_;
                    asm volatile(
                        "s_xor_b64 %[t0], %[s], %[e]\n\t"
                        "s_andn2_b64 %[t0], %[mine], %[t0]\n\t"
                        "s_and_b64 %[gf], %[t0], %[s]\n\t"
                        "s_or_b64 %[gf], %[gf], %[strad]\n\t"
                        "s_andn2_b64 %[gb], %[t0], %[s]\n\t"
                        "s_or_b64 %[gb], %[gb], %[strad]\n\t"
                        "s_or_b64 %[t0], %[gf], %[gb]\n\t"
                        "s_cselect_b32 %[any], 1, 0\n\t"
                        "s_and_b64 %[t1], %[t0], %[s]\n\t"
                        "s_bcnt1_i32_b64 %[nf], %[t1]\n\t"
                        "s_andn2_b64 %[t1], %[t0], %[s]\n\t"
                        "s_bcnt1_i32_b64 %[nb], %[t1]\n\t"
                        "s_cmp_ge_u32 %[nf], %[nb]\n\t"
                        "s_cselect_b32 %[ff], 1, 0\n\t"
                        "s_cselect_b32 %[c1], %[cf], %[cb]\n\t"
                        "s_cselect_b32 %[c2], %[cb], %[cf]\n\t"
                        "s_cselect_b64 %[i1], %[gf], %[gb]\n\t"
                        "s_cselect_b64 %[i2], %[gb], %[gf]\n\t"
                        "s_cmp_lg_u64 %[i2], 0\n\t"
                        "s_cselect_b32 %[push], 1, 0"
                        : [gf] "=&s"(go_f), [gb] "=&s"(go_b), [i1] "=&s"(in_first), [i2] "=&s"(in_second), [t0] "=&s"(t0_), [t1] "=&s"(t1_), [c1] "=&s"(c_first), [c2] "=&s"(c_second),
                          [ff] "=&s"(ff_), [push] "=&s"(push_), [any] "=&s"(any_), [nf] "=&s"(nf_), [nb] "=&s"(nb_)
                        : [s] "s"(s), [e] "s"(e), [mine] "s"(mine), [strad] "s"(strad), [cf] "s"(v[3]), [cb] "s"(v[4])
                        : "scc");
                    const bool front_first = ff_ != 0u;
                    const bool push = push_ != 0u;
                    const bool room = sp < wwords;
                    if (room && push) wstack[sp] = (c_second << 5) | (uint32_t)lev;
                    failed = failed || (push && !room);
                    descend = any_ != 0u && !failed;
                    sp += (push && descend) ? 1 : 0;
                    const pt_mask near_first = front_first ? s : PT_MNOT(s);
                    const pt_mask both = (push && descend) ? strad : 0ull;
                    if (lev < sav.top_levels) {
                        if (push && descend) { sav.path[3 * lev] = v[0]; sav.path[3 * lev + 1] = v[1]; sav.path[3 * lev + 2] = v[2]; }
                    } else if (both) pt_kd_sav_store(sav, lev, PT_LANES(near_first) ? end : start);
                    if (push && descend) {
                        code = PT_LANES(in_second) ? 1u : 0u;
                        if (both) {
                            code = PT_LANES(both & near_first) ? 2u : code;
                            code = PT_LANES(both & PT_MNOT(near_first)) ? 3u : code;
                            end = PT_LANES(both & near_first) ? plane_t : end;
                            start = PT_LANES(both & PT_MNOT(near_first)) ? plane_t : start;
                            if (!MESH) {
                                seg0c = (float)start; seg1c = (float)end;
                                seg0c = seg0c - fabsf(seg0c) * 2.4e-7f; seg1c = seg1c + fabsf(seg1c) * 2.4e-7f;
                            }
                        }
                    }
                }
#else
                const pt_mask same = mine & PT_MNOT(s ^ e);
                const pt_mask go_f = (same & s) | strad, go_b = (same & PT_MNOT(s)) | strad;
                // the child most lanes call near goes first (a lane's near side is the side of its range start)
                const bool front_first = PT_POPC((go_f | go_b) & s) >= PT_POPC((go_f | go_b) & PT_MNOT(s));
                const uint32_t c_first = front_first ? v[3] : v[4], c_second = front_first ? v[4] : v[3];
                const pt_mask in_first = front_first ? go_f : go_b, in_second = front_first ? go_b : go_f;
                const bool push = in_second != 0ull;
                const bool room = sp < wwords;
                if (room && push) wstack[sp] = (c_second << 5) | (uint32_t)lev;  // one word: the child and the split's level
                failed = failed || (push && !room);
                descend = (go_f | go_b) != 0ull && !failed;
                sp += (push && descend) ? 1 : 0;
                // the lanes' own bookkeeping, without branches: both children (straddling) - one bound becomes plane_t and goes to the
                // slot, code 2 (the slot holds the end) / 3 (the start); the second child only - code 1; else 0. Lanes whose slot is not
                // read later may write it too.
                const pt_mask near_first = front_first ? s : PT_MNOT(s);
                const pt_mask both = (push && descend) ? strad : 0ull;
                if (lev < sav.top_levels) {  // a top level: no slot - the path table gets the split's plane and axis (every lane writes the same words)
                    if (push && descend) { sav.path[3 * lev] = v[0]; sav.path[3 * lev + 1] = v[1]; sav.path[3 * lev + 2] = v[2]; }
                } else if (both) pt_kd_sav_store(sav, lev, PT_LANES(near_first) ? end : start);
                // (behind wave-uniform branches since round 5: most splits below the top levels push nothing - every lane is on one side - and then there is nothing to select;
                // the walk is bound by instruction issue, big-scene 27.55 -> 27.27 ms, c28)
                uint32_t code = 0u;
                if (push && descend) {
                    code = PT_LANES(in_second) ? 1u : 0u;
                    if (both) {
                        code = PT_LANES(both & near_first) ? 2u : code;
                        code = PT_LANES(both & PT_MNOT(near_first)) ? 3u : code;
                        end = PT_LANES(both & near_first) ? plane_t : end;
                        start = PT_LANES(both & PT_MNOT(near_first)) ? plane_t : start;
                    }
                }
#endif
                if (descend) {
                    const int sh = 2 * (lev & 15);
                    if (lev < 16) codes_lo = (codes_lo & ~(3u << sh)) | (code << sh);
                    else codes_hi = (codes_hi & ~(3u << sh)) | (code << sh);
                    in = in_first; cur = c_first; lev++;
                }
            } else if (mine) {
                // ---- a leaf: ray.rs:87-99 fold over the leaf's nodes in the reference's order with a strictly shrinking end
                if (STATS && PT_LANES(mine)) cnt->n_leaf++;
                PT_WAVE_COUNT(5);
                const uint32_t first = v[5], count = v[6];
                PtHit lb; lb.t = end; lb.node = PT_NO_HIT; lb.sub = 0;
                pt_mask found = 0ull;
                pt_mask want = mine;  // a shadow ray is done with its first hit
                const void* const info_base = pt_pin_ptr(sc.info);
                const void* const inv_base = pt_pin_ptr(sc.inv);
                for (uint32_t i = 0; i < count; i++) {
                    // the reference and its cull box in one scalar fetch: {flattened node, 0, the node's padded world box as 6 f32 rounded outward}
                    const pt_u32x8 ref = pt_sload8_off(ref_base, (first + i) << 5);
                    PT_WAVE_COUNT(6);  // -DPT_DIAG: leaf references looked at, per wavefront (per lane: n_bbox)
                    const uint32_t item = ref[0];
                    pt_mask test = want;
                    if (cull & 2u) {  // a node whose box the lane's segment does not reach cannot report a hit in it
                        const float lo[3] = {pt_f32_of(ref[2]), pt_f32_of(ref[3]), pt_f32_of(ref[4])}, hi[3] = {pt_f32_of(ref[5]), pt_f32_of(ref[6]), pt_f32_of(ref[7])};
                        if (STATS && PT_LANES(want)) cnt->n_bbox++;
                        test &= pt_slab_seg_pk_m(lo, hi, q, seg0, seg1);
                    }
                    if (!test) continue;
                    PT_WAVE_COUNT(7);  // -DPT_DIAG: exact tests, per wavefront (per lane: n_analytic)
                    // the node's record in one round trip through the scalar cache: {type, data, flags, material} and rows 0..2 of its inverse
                    pt_u32x4 info;
                    pt_u32x16 ma;
                    pt_u32x8 mb;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("s_load_dwordx4 %0, %3, %5\n\ts_load_dwordx16 %1, %4, %6\n\ts_load_dwordx8 %2, %4, %7\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&s"(info), "=&s"(ma), "=&s"(mb) : "s"(info_base), "s"(inv_base), "s"(item << 4), "s"(item * 96u), "s"(item * 96u + 64u) : "memory");
#else
                    info = *reinterpret_cast<const pt_u32x4*>(static_cast<const char*>(info_base) + ((size_t)item << 4));
                    ma = *reinterpret_cast<const pt_u32x16*>(static_cast<const char*>(inv_base) + (size_t)item * 96u);
                    mb = *reinterpret_cast<const pt_u32x8*>(static_cast<const char*>(inv_base) + (size_t)item * 96u + 64u);
#endif
                    const uint32_t type = info[0], data = info[1];
                    double mm[12];
#pragma unroll
                    for (int k = 0; k < 8; k++) mm[k] = pt_f64_of(ma[2 * k], ma[2 * k + 1]);
#pragma unroll
                    for (int k = 0; k < 4; k++) mm[8 + k] = pt_f64_of(mb[2 * k], mb[2 * k + 1]);
                    const PtRay local = pt_ray_to_local(mm, ray);  // flat_scene.rs:74
                    const bool test_l = PT_LANES(test);
                    if (STATS && test_l) cnt->n_analytic++;
                    bool hit = false;
                    if (MESH && (type == PT_MESH || type == PT_KDMESH)) {
                        const PtMeshInfo* mi = sc.meshes + data;
                        double bi[12];
                        pt_u32x4 head;  // {tri_first, tri_count, blas_root, kd_root}: one round trip with the box inverse
                        pt_sload_mat12_x4(mi->bbox_inv, bi, head);
                        if (KDMESH && type == PT_KDMESH && (int32_t)head[3] >= 0) {  // the reference's own triangle tree (quirk Q3), per lane
                            if (test_l) {
                                double t; uint32_t tri = 0;
                                if (pt_kdmesh_hit<STATS>(sc, *mi, local, start, pt_cand_end(lb, item, 0), lane_stk, 0, &t, &tri, cnt)) { lb.t = t; lb.node = item; lb.sub = tri; hit = true; }
                            }
                        } else {  // mesh.rs:146-155: box test, then the triangles (also a KDMesh without a tree of its own: PORTRAYER_KDMESH_AS_MESH)
                            const uint32_t root = head[2];
                            if (STATS && test_l) cnt->n_bbox++;
                            if (root == PT_REF_EMPTY) continue;
                            const bool inside = test_l && pt_bbox_test_hit(bi, local, start, pt_cand_end(lb, item, 0));
                            if (!pt_any(inside)) continue;
                            if (!pt_packet_mesh_below_kd<STATS>(sc, item, root, head[1], local, inside, start, PT_LANES(any_m), lb, hit, wstack + sp, wwords - sp, cnt)) failed = true;
                        }
                    } else if (test_l) {
                        double t; uint32_t part = 0;
                        if (type == PT_TRIANGLE) {  // stand-alone triangle, stored after the mesh triangles
                            double beta, gamma;
                            if (STATS) cnt->n_tri++;
                            hit = pt_triangle_hit(sc.tri_v + 9 * (size_t)data, local, start, pt_cand_end(lb, item, data), &t, &beta, &gamma);
                            part = data;
                        } else {
                            hit = pt_unit_prim_hit(type, local, start, pt_cand_end(lb, item, 0), &t, &part);
                        }
                        if (hit) { lb.t = t; lb.node = item; lb.sub = part; }
                    }
                    const pt_mask hit_m = PT_BALLOT(hit);
                    found |= hit_m;
                    want &= PT_MNOT(hit_m & any_m);
                    // the segment has shrunk: later references of this leaf are culled against the new end
                    if (hit_m) { const float s1 = (float)lb.t; seg1 = PT_LANES(hit_m) ? s1 + fabsf(s1) * 2.4e-7f : seg1; }
                }
                if (found) {  // (start <= lb.t < best.t by the admission test above)
                    const bool f = PT_LANES(found);
                    best.t = f ? lb.t : best.t; best.node = f ? lb.node : best.node; best.sub = f ? lb.sub : best.sub;
                    alive &= PT_MNOT(found & any_m);
                }
            }
        }
        if (descend) continue;
        // ---- the next pending subtree: the second child of the split at level L. (The way out of the walk is tested at the very end of
        // the body and everything before it runs either way - reading slot 0 of an empty stack is harmless -: on a path that leaves the loop
        // early the node index would be undefined, the compiler gives undefined values VECTOR registers, and its SGPR-copy fixing then moves
        // the whole chain of the node index to the vector side, where the scalar load cannot take it.)
        const bool done = failed || alive == 0ull || sp == 0;
        sp -= done ? 0 : 1;
        const uint32_t entry = PT_UNIFORM_U32(wstack[sp]);
        cur = entry >> 5;
        const int L = (int)(entry & 31u);
        if (L >= sav.top_levels) {
            for (int k = lev - 1; k > L; k--) {  // the finished levels below it: put the replaced bounds back
                const uint32_t c = ((k < 16 ? codes_lo : codes_hi) >> (2 * (k & 15))) & 3u;
                const pt_mask c2m = PT_U32_EQ(c, 2u), c3m = PT_U32_EQ(c, 3u);
                if (c2m | c3m) {
                    const double sv = pt_kd_sav_load(sav, k);  // (lanes whose slot holds nothing read it too: not used)
                    end = PT_LANES(c2m) ? sv : end;
                    start = PT_LANES(c3m) ? sv : start;
                }
            }
        }
        {
            const int sh = 2 * (L & 15);
            const uint32_t c = ((L < 16 ? codes_lo : codes_hi) >> sh) & 3u;
            const pt_mask c2m = PT_U32_EQ(c, 2u), c3m = PT_U32_EQ(c, 3u);
            if (L >= sav.top_levels && (c2m | c3m)) {
                // had [start, plane_t) (c == 2, the slot holds the end): now [plane_t, end), the slot keeps the start for the way back up;
                // had [plane_t, end) (c == 3, the slot holds the start): now [start, plane_t), the slot keeps the end
                const double sv = pt_kd_sav_load(sav, L);
                pt_kd_sav_store(sav, L, PT_LANES(c2m) ? start : end);
                const double ns = PT_LANES(c2m) ? end : (PT_LANES(c3m) ? sv : start);
                const double ne = PT_LANES(c2m) ? sv : (PT_LANES(c3m) ? start : end);
                start = ns; end = ne;
            }
            in = PT_MNOT(PT_U32_EQ(c, 0u));
            const uint32_t c2 = PT_LANES(c2m) ? 3u : (PT_LANES(c3m) ? 2u : 0u);
            if (L < 16) codes_lo = (codes_lo & ~(3u << sh)) | (c2 << sh);
            else codes_hi = (codes_hi & ~(3u << sh)) | (c2 << sh);
        }
        if (L < sav.top_levels && !done) {
            // A top level: the range of the second child from the codes of the levels 0 .. L alone (see PtKdSav) - end = the plane parameter of the deepest
            // level with code 2, else infinity; start = that of the deepest level with code 3, else epsilon. Deepest first, until every lane has both.
            pt_mask need_e = in, need_s = in;
            for (int j = L; j >= 0 && (need_e | need_s); j--) {
                const uint32_t cj = ((j < 16 ? codes_lo : codes_hi) >> (2 * (j & 15))) & 3u;
                const pt_mask e_here = PT_U32_EQ(cj, 2u) & need_e, s_here = PT_U32_EQ(cj, 3u) & need_s;
                if (!(e_here | s_here)) continue;
                const uint32_t p0 = PT_UNIFORM_U32(sav.path[3 * j]), p1 = PT_UNIFORM_U32(sav.path[3 * j + 1]), ax = PT_UNIFORM_U32(sav.path[3 * j + 2]);
                const double plane = pt_f64_of(p0, p1);
                double tj;
                if (ax == 0u) tj = pt_kd_plane_t(ray.o.x, ray.d.x, yx, okx, plane, e_here | s_here);
                else if (ax == 1u) tj = pt_kd_plane_t(ray.o.y, ray.d.y, yy, oky, plane, e_here | s_here);
                else tj = pt_kd_plane_t(ray.o.z, ray.d.z, yz, okz, plane, e_here | s_here);
                end = PT_LANES(e_here) ? tj : end;
                start = PT_LANES(s_here) ? tj : start;
                need_e &= PT_MNOT(e_here); need_s &= PT_MNOT(s_here);
            }
            end = PT_LANES(need_e) ? (double)INFINITY : end;
            start = PT_LANES(need_s) ? (double)PT_EPSILON : start;
        }
        lev = L + 1;
        if (!MESH) {
            seg0c = (float)start; seg1c = (float)end;
            seg0c = seg0c - fabsf(seg0c) * 2.4e-7f; seg1c = seg1c + fabsf(seg1c) * 2.4e-7f;
        }
        if (done) break;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : : "s"(cur), "s"(lev), "s"(sp));  // (live, and in scalar registers, on the way out: see above)
#endif
    if (failed) {  // never expected (pt_scene_upload sizes the stack); recorded unconditionally so that a render whose results would be wrong cannot return PT_OK
#if defined(__HIP_DEVICE_COMPILE__)
        if (overflow) atomicOr(overflow, steps > PT_KD_WALK_STEPS_MAX ? 4u : 1u);  // 4: the watchdog
#endif
        if (STATS) cnt->stack_overflow++;
        if (has_ray) best.node = PT_NO_HIT;
    }
}
