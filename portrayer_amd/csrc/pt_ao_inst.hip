// One traversal mode's instantiations of pt_ao_kernel - the ambient-occlusion pass (pt_ao, include/portrayer_hip.h) in its two work layouts - and
// their launcher. Compiled once per mode, -DPT_INST_MODE=1..9 (Makefile: pt_ao_m<mode>.o), through the same check / repair of the assembly as every pass.
//
// A lane makes its ray in registers from the point, its normal and two tables of constants (pt_ao.h: the contract), walks it as pt_segments_kernel walks a
// caller's ray with t_max = radius and any_hit = 1, and the wavefront counts: no ray, origin or direction is ever in memory. Like pt_segments_inst.hip this
// unit's walks of the flat_scene and hierarchical semantics start at the lane's bound (PT_WALK_ENTRY_T) and prune with it, with the same two exceptions (a
// KDMesh instance's own tree, a Mesh instance's box test); in the k-d semantics the walk is the unbounded nearest-hit walk, filtered by hit.t < radius.
#define PT_WALK_ENTRY_T(best) (best).t
#define PT_WALK_ENTRY_TM(best) pt_tmax32((best).t)
#define PT_WALK_KDMESH_HIT(STATS, HIER, sc, mi, lr, best, node, lane_stk, t, tri, cnt) pt_kdmesh_hit_filtered<STATS, HIER>(sc, mi, lr, best, node, lane_stk, t, tri, cnt)
#define PT_WALK_MESH_BOX_END(HIER, sc, best, node) ((best).node == PT_NO_HIT ? (double)INFINITY : pt_cand_end_in<HIER>(sc, best, node, 0))
#include "pt_render_kernel.h"
#include "pt_ao_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

// Work item w of the two layouts (both give every point the same bits: no walk result depends on which rays share a wavefront):
//   PT_AO_POINT_MAJOR   64 / S consecutive points x S samples, lane l = (point l / S, sample l % S). The count is a ballot's population inside the point's group of
//                       lanes; the bent normal is summed by the group's first lane from the wavefront's LDS column of directions, in sample order - the pattern
//                       of the render kernels' chunk sums.
//   PT_AO_SAMPLE_MAJOR  64 consecutive points, one walk per sample k = 0 .. S - 1; the count accumulates in a register, the bent normal in the lane's own LDS slots.
// Invalid points (pt_ao_valid), rays pt_segments would not trace and lanes past n are idle lanes: a zero ray, traced = false, as in pt_segments_kernel.
// Persistent wavefronts, one item at a time from the interleaved queues, stacks continuing in the lanes' HBM columns: as in pt_segments_kernel.
template <int MODE, int LAYOUT>
__global__ void __launch_bounds__(PT_BLOCK, pt_ao_waves(MODE)) pt_ao_kernel(PtAoArgs a1) {
    constexpr bool KD = MODE == PT_MODE_KD || MODE == PT_MODE_KD_NOMESH || MODE == PT_MODE_KD_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a1.r;
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
    const double radius = a1.radius;
    const unsigned S = a1.samples, sh = a1.log2_samples;
    // The wavefront's columns behind the block's stack area (pt_ao_frame_bytes), component-major, 64 doubles each: the lanes' directions (3) and, sample-major, their
    // sums so far (3 more). Nothing of the walks reaches there.
    double* const col = (double*)(pt_lds + (size_t)a.stack_lds_cap * PT_BLOCK) + (size_t)(threadIdx.x >> 6) * (LAYOUT == PT_AO_POINT_MAJOR ? 192 : 384);

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

        const uint64_t p = LAYOUT == PT_AO_POINT_MAJOR ? ((uint64_t)w << (6u - sh)) + (lane >> sh) : (uint64_t)w * 64u + lane;
        const bool mine = p < a1.n;
        bool valid = false;
        if (mine) {
            const double* P = a1.positions + 3 * (size_t)p;
            const double* N = a1.normals + 3 * (size_t)p;
            valid = pt_ao_valid(pt_v3(P[0], P[1], P[2]), pt_v3(N[0], N[1], N[2]));
        }
        unsigned count = 0;
        PtVec3 sum = pt_v3(0.0, 0.0, 0.0);
        if (LAYOUT == PT_AO_SAMPLE_MAJOR && a1.bent) col[192 + lane] = col[256 + lane] = col[320 + lane] = 0.0;
        const unsigned k_end = LAYOUT == PT_AO_POINT_MAJOR ? 1u : S;
        for (unsigned kk = 0; kk < k_end; kk++) {
            const unsigned k = LAYOUT == PT_AO_POINT_MAJOR ? (lane & (S - 1u)) : kk;
            PtRay ray;
            ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
            if (valid) {  // (point and normal are read again per sample: 48 bytes from the cache, not twelve registers held across the walk)
                const double* P = a1.positions + 3 * (size_t)p;
                const double* N = a1.normals + 3 * (size_t)p;
                pt_ao_ray(a1.set, pt_v3(P[0], P[1], P[2]), pt_v3(N[0], N[1], N[2]), a1.set.first_index + p, k, &ray.o, &ray.d);
            }
            // What the bent normal sums, traced or not, waits in the lane's LDS slots while the walk runs: six registers the walk does not have to carry.
            if (a1.bent) { col[lane] = ray.d.x; col[64 + lane] = ray.d.y; col[128 + lane] = ray.d.z; }  // (wave-uniform)
            const bool traced = valid && pt_segments_traced(ray, radius);
            if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
            PtHit hit;
            hit.t = traced ? radius : (double)INFINITY;  // the bound the lane enters the walk with (the k-d walk resets it)
            hit.node = PT_NO_HIT; hit.sub = 0;
            if (__any(traced)) pt_trace_wave<MODE, false>(a, ray, traced, !KD, hit, stk, pt_lds, &cnt);
            const bool occ = traced && hit.node != PT_NO_HIT && (!KD || hit.t < radius);

            if (LAYOUT == PT_AO_SAMPLE_MAJOR) {  // the lane's own slots: the sum so far beside the direction
                if (occ) count++;
                else if (valid && a1.bent) { col[192 + lane] += col[lane]; col[256 + lane] += col[64 + lane]; col[320 + lane] += col[128 + lane]; }
                continue;
            }
            const unsigned long long bal = __ballot(occ);
            if (a1.bent) {  // the group's directions are read by its first lane: same wavefront, program order suffices
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            if (k == 0) {  // the group's first lane: its lanes are lane .. lane + S - 1
                const unsigned long long grp = (bal >> lane) & (S == 64u ? ~0ull : (1ull << S) - 1ull);
                count = (unsigned)__popcll(grp);
                if (a1.bent && valid)
                    for (unsigned j = 0; j < S && j < 64u; j++)  // (bounded by a constant as well)
                        if (!((grp >> j) & 1ull)) sum = sum + pt_v3(col[lane + j], col[64 + lane + j], col[128 + lane + j]);
            }
            if (a1.bent) __builtin_amdgcn_wave_barrier();  // the column is free for the next item
        }
        if (LAYOUT == PT_AO_SAMPLE_MAJOR && a1.bent) sum = pt_v3(col[192 + lane], col[256 + lane], col[320 + lane]);
        if (!mine || (LAYOUT == PT_AO_POINT_MAJOR && (lane & (S - 1u)) != 0)) continue;  // one lane per point writes
        if (a1.occluded) a1.occluded[p] = count;
        if (a1.valid) a1.valid[p] = valid ? 1 : 0;
        if (a1.bent) { double* o = a1.bent + 3 * (size_t)p; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
    }
}

// Launch (or, with launch = false, only size) the pass in one layout: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_ao_launch(const PtAoArgs& a, int layout, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.r.stack_lds_cap * PT_BLOCK * 4 + pt_ao_frame_bytes(layout);  // the traversal stack area, and the wavefronts' columns behind it
    if (layout == PT_AO_POINT_MAJOR) return pt_launch_kernel_args<&pt_ao_kernel<MODE, PT_AO_POINT_MAJOR>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<&pt_ao_kernel<MODE, PT_AO_SAMPLE_MAJOR>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}

hipError_t PT_INST_CAT(pt_ao_launch_mode_, PT_INST_MODE)(const PtAoArgs& a, int layout, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_ao_launch<PT_INST_MODE>(a, layout, n_cu, stream, grid, launch);
}
