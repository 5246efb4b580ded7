// One traversal mode's instantiation of pt_direct_kernel - the direct-light pass (pt_direct, include/portrayer_hip.h) - and its launcher. Compiled once
// per mode, -DPT_INST_MODE=1..9 (Makefile: pt_direct_m<mode>.o), through the same check / repair of the assembly as every pass.
//
// A lane makes its shadow ray in registers from the point, its normal and the light's record (pt_direct.h: the contract), walks it as pt_segments_kernel walks a
// caller's ray with that t_max and any_hit = 1, and adds the light's term to its own sum if nothing was met: no ray, origin, direction or term is ever in memory.
// Like pt_segments_inst.hip and pt_ao_inst.hip this unit's walks of the flat_scene and hierarchical semantics start at the lane's bound (PT_WALK_ENTRY_T) and prune
// with it, with the same two exceptions (a KDMesh instance's own tree, a Mesh instance's box test); in the k-d semantics the walk is the unbounded nearest-hit
// walk, filtered by hit.t < t_max.
#define PT_WALK_ENTRY_T(best) (best).t
#define PT_WALK_ENTRY_TM(best) pt_tmax32((best).t)
#define PT_WALK_KDMESH_HIT(STATS, HIER, sc, mi, lr, best, node, lane_stk, t, tri, cnt) pt_kdmesh_hit_filtered<STATS, HIER>(sc, mi, lr, best, node, lane_stk, t, tri, cnt)
#define PT_WALK_MESH_BOX_END(HIER, sc, best, node) ((best).node == PT_NO_HIT ? (double)INFINITY : pt_cand_end_in<HIER>(sc, best, node, 0))
#include "pt_render_kernel.h"
#include "pt_direct_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

// A light's 15 doubles at a wave-uniform address, in one round trip through the scalar cache (pt_sload_mat12's pattern, 120 bytes).
PT_HD void pt_direct_sload_light(const double* p, double m[15]) {
    pt_u32x16 a;
    pt_u32x8 b;
    pt_u32x4 c;
    uint64_t d;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx8 %1, %4, 0x40\n\ts_load_dwordx4 %2, %4, 0x60\n\ts_load_dwordx2 %3, %4, 0x70\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(pt_uniform_ptr(p)) : "memory");
#else
    a = *reinterpret_cast<const pt_u32x16*>(p);
    b = *reinterpret_cast<const pt_u32x8*>(reinterpret_cast<const char*>(p) + 64);
    c = *reinterpret_cast<const pt_u32x4*>(reinterpret_cast<const char*>(p) + 96);
    d = *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(p) + 112);
#endif
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = pt_f64_of(a[2 * k], a[2 * k + 1]);
#pragma unroll
    for (int k = 0; k < 4; k++) m[8 + k] = pt_f64_of(b[2 * k], b[2 * k + 1]);
    m[12] = pt_f64_of(c[0], c[1]);
    m[13] = pt_f64_of(c[2], c[3]);
    m[14] = pt_f64_of((uint32_t)d, (uint32_t)(d >> 32));
}

// Work item w: 64 consecutive points, lane = point. The wavefront loops over the lights and, for an area light, over its samples: one walk for the 64 rays from
// neighbouring points to one light. The light's record is wave-uniform and is fetched again in front of every walk, so that none of it has to live across one; the
// lane's term waits in its LDS slots while the walk runs, beside its sum so far (pt_ao_kernel's sample-major columns), and the lane adds in contract order: no
// cross-lane reduction, and no result depends on which rays share a wavefront. A sample for which no lane of the wavefront casts a ray is skipped
// without a walk. Invalid points (pt_direct_valid), samples that cast no ray and lanes past n are idle lanes: a zero ray, traced = false, as in pt_segments_kernel.
// Persistent wavefronts, one item at a time from the interleaved queues, stacks continuing in the lanes' HBM columns: as in pt_segments_kernel.
template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK, pt_direct_waves(MODE)) pt_direct_kernel(PtDirectArgs a1) {
    constexpr bool KD = MODE == PT_MODE_KD || MODE == PT_MODE_KD_NOMESH || MODE == PT_MODE_KD_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a1.r;
    const PtSceneView& sc = a.scene;
    const uint32_t lane_global = blockIdx.x * PT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    PtStackSpill stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = a.stack_lds_cap;
    stk.total = a.scene.stack_cap;
    stk.gbase = a.stack_spill + lane_global;
    stk.gstride = a.n_lanes;
    stk.overflow = a.overflow_flag;
    PtCounters cnt;  // (the walks take a pointer; nothing is counted)
    const unsigned S = a1.set.samples;
    // The wavefront's columns behind the block's stack area (pt_direct_frame_bytes), component-major, 64 doubles each: the lanes' terms (3) and their sums so far
    // (3 more). Nothing of the walks reaches there.
    double* const col = (double*)(pt_lds + (size_t)a.stack_lds_cap * PT_BLOCK) + (size_t)(threadIdx.x >> 6) * 384;

    unsigned q_next = blockIdx.x % a.fine_queues, q_end = 0;
    for (;;) {
        unsigned w;
        for (;;) {
            unsigned idx = 0;
            if (lane == 0) idx = atomicAdd(a.work_queues + q_next * PT_QUEUE_STRIDE, 1u);
            idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
            const unsigned long long pos = (unsigned long long)idx * a.fine_queues + q_next;
            if (pos < a.n_items) { w = (unsigned)pos; q_end = 0; break; }
            q_next = q_next + 1u == a.fine_queues ? 0u : q_next + 1u;
            if (++q_end == a.fine_queues) { w = 0xFFFFFFFFu; break; }
        }
        if (w == 0xFFFFFFFFu) break;

        const uint64_t p = (uint64_t)w * 64u + lane;
        const bool mine = p < a1.n;
        bool valid = false;
        if (mine) {
            const double* P = a1.positions + 3 * (size_t)p;
            const double* N = a1.normals + 3 * (size_t)p;
            valid = pt_direct_valid(pt_v3(P[0], P[1], P[2]), pt_v3(N[0], N[1], N[2]));
        }
        unsigned lit = 0;
        col[192 + lane] = col[256 + lane] = col[320 + lane] = 0.0;
        const uint32_t n_lights = __any(valid) ? sc.n_lights : 0u;  // (a wavefront of invalid points visits no light)
        uint32_t j = 0;                                             // area lights in front of light li
        for (uint32_t li = 0; li < n_lights; li++) {
            bool point = false;  // (known after the first fetch of the record: a point light has one sample)
            for (unsigned k = 0; k < (point ? 1u : S); k++) {
                double light[15];
                pt_direct_sload_light(sc.lights + 15 * (size_t)li, light);
                point = PT_UNIFORM_U32(pt_direct_is_point_light(light) ? 1u : 0u) != 0u;
                PtRay ray;
                ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
                double t_max = 0.0;
                bool traced = false;
                if (valid) {  // (point and normal are read again per sample: 48 bytes from the cache, not twelve registers held across the walk)
                    const double* P = a1.positions + 3 * (size_t)p;
                    const double* N = a1.normals + 3 * (size_t)p;
                    PtVec3 o, nrm, term;
                    pt_direct_point(a1.set, pt_v3(P[0], P[1], P[2]), pt_v3(N[0], N[1], N[2]), &o, &nrm);
                    const PtVec3 lpos = pt_direct_light_position(a1.set, light, j, a1.set.first_index + p, k);
                    traced = pt_direct_sample(a1.set, o, nrm, lpos, light, &ray.d, &t_max, &term);
                    if (traced) ray.o = o;  // (else what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic)
                    col[lane] = term.x; col[64 + lane] = term.y; col[128 + lane] = term.z;
                }
                PtHit hit;
                hit.t = traced ? t_max : (double)INFINITY;  // the bound the lane enters the walk with (the k-d walk resets it)
                hit.node = PT_NO_HIT; hit.sub = 0;
                if (__any(traced)) pt_trace_wave<MODE, false>(a, ray, traced, !KD, hit, stk, pt_lds, &cnt);
                const bool occ = hit.node != PT_NO_HIT && (!KD || hit.t < t_max);
                if (traced && !occ) {  // the lane's own slots: the sum so far beside the term; a point light's one sample stands for all S
                    const unsigned reps = point ? S : 1u;
                    const PtVec3 term = pt_v3(col[lane], col[64 + lane], col[128 + lane]);
                    PtVec3 sum = pt_v3(col[192 + lane], col[256 + lane], col[320 + lane]);
                    for (unsigned r = 0; r < reps; r++) sum = sum + term;
                    col[192 + lane] = sum.x; col[256 + lane] = sum.y; col[320 + lane] = sum.z;
                    lit += reps;
                }
            }
            if (!point) j++;
        }
        if (!mine) continue;  // (a lane past n: nothing to write)
        if (a1.sum) { double* o = a1.sum + 3 * (size_t)p; o[0] = col[192 + lane]; o[1] = col[256 + lane]; o[2] = col[320 + lane]; }
        if (a1.lit) a1.lit[p] = lit;
        if (a1.valid) a1.valid[p] = valid ? 1 : 0;
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_direct_launch(const PtDirectArgs& a, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.r.stack_lds_cap * PT_BLOCK * 4 + pt_direct_frame_bytes();  // the traversal stack area, and the wavefronts' columns behind it
    return pt_launch_kernel_args<&pt_direct_kernel<MODE>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}

hipError_t PT_INST_CAT(pt_direct_launch_mode_, PT_INST_MODE)(const PtDirectArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_direct_launch<PT_INST_MODE>(a, n_cu, stream, grid, launch);
}
