// The bounded-segment ray queries (pt_segments, include/portrayer_hip.h): pt_rays_kernel (pt_rays.h) plus one 8-byte load per ray, its t_max. Per ray the
// result is pt_rays' restricted to hits with PT_EPSILON <= t < t_max: the nearest such hit, or (any = true) whether there is one. A ray whose range is empty
// (t_max NaN or <= PT_EPSILON) is not traced, like the rays pt_rays_traced rejects: an idle lane that reports a miss.
//
// flat_scene and hierarchical semantics: the crate's ray_cast(&ray, &mut Range {start: EPSILON, end: t_max}). The lane enters the wavefront's walk with
// hit.t = t_max and hit.node = PT_NO_HIT, and the walk neither resets that bound nor starts its f32 image at infinity (PT_WALK_ENTRY_T / PT_WALK_ENTRY_TM,
// defined by pt_segments_inst.hip before anything is included): boxes beyond the bound are never entered, pt_cand_end / pt_cand_end_in give every candidate the
// half-open range [EPSILON, t_max), a mesh's box test (bounding_box.rs:104-116) gets the same range, exact ties keep their winner, and an occlusion walk still
// ends at the first hit inside the range. Whatever the walk reports is therefore in range; a miss leaves hit.node = PT_NO_HIT. Two tests are the exception,
// because their outcome for a hit just inside the bound depends on more than the exact comparison t < t_max: a KDMesh instance's own triangle k-d tree (its side
// classification reads the range's end, pt_kdmesh_hit) and a Mesh instance's box test (the box's entry parameter is rounded differently from a triangle's t). While
// the lane has found nothing both get [EPSILON, inf), and a KDMesh's hit is kept iff t < t_max (PT_WALK_KDMESH_HIT, PT_WALK_MESH_BOX_END in pt_walk_wave.h) - the
// unbounded result, filtered, as in the k-d semantics below.
// k-d semantics: by definition the UNBOUNDED walk's result, filtered (the crate's own bounded range would enter the split classification, node.rs:121). The
// walk (pt_trace_packet_kd, untouched) resets the bound itself and runs as a nearest-hit walk also for any = true - an occlusion walk may stop at an occluder
// beyond t_max while a nearer one sits in another leaf - and the kernel compares hit.t < t_max afterwards. No pruning: the known cost of these semantics.
#pragma once

#ifndef PT_WALK_ENTRY_T
#error "pt_segments.h: define PT_WALK_ENTRY_T / PT_WALK_ENTRY_TM first (pt_segments_inst.hip) - with the defaults of pt_walk_wave.h the walks would ignore t_max"
#endif

#include "pt_render_kernel.h"
#include "pt_segments_inst.h"

template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK, pt_segments_waves(MODE)) pt_segments_kernel(PtSegmentsArgs a1) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    constexpr bool MESHES = !(MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_KD_NOMESH);
    constexpr bool KD = MODE == PT_MODE_KD || MODE == PT_MODE_KD_NOMESH || MODE == PT_MODE_KD_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRaysArgs& a0 = a1.q;
    const PtRenderArgs& a = a0.r;
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
    const bool any = a0.any != 0;

    // items are handed out one at a time from interleaved queues (pt_rays_kernel): item idx * N + q from queue q
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
        const uint64_t slot = (uint64_t)w * 64u + lane;
        const bool mine = slot < a0.n;
        size_t i = (size_t)slot;
        if (mine && a0.perm) i = a0.perm[slot];  // (< n: a permutation of 0 .. n - 1)
        PtRay ray;
        ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
        double t_max = 0.0;
        if (mine) {
            const double* o = a0.origins + 3 * i;
            const double* d = a0.directions + 3 * i;
            ray.o = pt_v3(o[0], o[1], o[2]);
            ray.d = pt_v3(d[0], d[1], d[2]);
            t_max = a1.t_max[i];
        }
        const bool traced = mine && pt_segments_traced(ray, t_max);
        if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
        PtHit hit;
        hit.t = traced ? t_max : (double)INFINITY;  // the bound the lane enters the walk with (the k-d walk resets it)
        hit.node = PT_NO_HIT; hit.sub = 0;
        if (__any(traced)) pt_trace_wave<MODE, false>(a, ray, traced, KD ? false : any, hit, stk, pt_lds, &cnt);
        if (!mine) continue;  // (a lane past n: nothing to write)

        const bool ok = traced && hit.node != PT_NO_HIT && (!KD || hit.t < t_max);
        if (a0.occluded) a0.occluded[i] = ok ? 1 : 0;
        if (any) continue;  // which occluder the walk met first depends on the schedule: only the flag is a result
        if (a0.t) a0.t[i] = ok ? hit.t : INFINITY;
        if (a0.node) a0.node[i] = ok ? (int32_t)hit.node : -1;
        if (a0.sub || a0.material) {
            int32_t sub = -1, mat = -1;
            if (ok) {
                const uint32_t* info = sc.info + 4 * (size_t)hit.node;
                mat = (int32_t)info[3];
                sub = 0;
                if (MESHES && (info[0] == PT_MESH || info[0] == PT_KDMESH)) sub = (int32_t)(hit.sub - sc.meshes[info[1]].tri_first);  // hit.sub: the triangle's index over all meshes
            }
            if (a0.sub) a0.sub[i] = sub;
            if (a0.material) a0.material[i] = mat;
        }
        if (a0.position || a0.normal) {  // (wave-uniform: no world transform is computed that nobody asked for)
            PtVec3 P = pt_v3(0.0, 0.0, 0.0), N = P;
            if (ok) {
                uint32_t mat, ftag;
                pt_hit_surface<false, HIER>(sc, ray, hit, &P, &N, &mat, &ftag);
            }
            if (a0.position) { double* o = a0.position + 3 * i; o[0] = P.x; o[1] = P.y; o[2] = P.z; }
            if (a0.normal) { double* o = a0.normal + 3 * i; o[0] = N.x; o[1] = N.y; o[2] = N.z; }
        }
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_segments_launch(const PtSegmentsArgs& a, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.q.r.stack_lds_cap * PT_BLOCK * 4;  // the traversal stack area alone
    return pt_launch_kernel_args<&pt_segments_kernel<MODE>>(lds, a, a.q.r.n_items, a.q.r.grid_share, n_cu, stream, grid_out, launch);
}
