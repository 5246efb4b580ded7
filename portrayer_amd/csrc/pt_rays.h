// The ray-query pass (pt_rays, include/portrayer_hip.h): rays the CALLER supplies - origin and direction in world space, 48 bytes each - and per ray
// either its nearest hit over [PT_EPSILON, inf) (t, flattened node, triangle inside its mesh, material index; where asked for, the world-space point
// and the normalised world-space normal: what pt_aov writes per pixel, computed by the same code) or whether anything is in the way at all
// (any = true: the shadow rays' question, material.rs:171-179).
//
// Work item: one wavefront = 64 consecutive ray indices, or with a permutation (reorder = 1, pt_rays_sort.hip) 64 consecutive entries of it; every
// result is written at the ray's own index. Lanes past n and rays that are not traced (pt_rays_traced) carry no ray, as idle lanes do in the render
// kernels: they take no part in the walk's ballots, and a ray that is not traced reports a miss. Nothing of the tracing is new: the walk is the render
// kernels' pt_trace_wave, the surface is pt_hit_surface with the material maps compiled out. No result of the walks depends on which rays share a
// wavefront - this pass is the caller that mixes octants, origins and axis-parallel directions freely inside one.
//
// Persistent wavefronts, one item at a time from 16 interleaved queues, stacks continuing in the lanes' HBM columns: as in pt_aov_kernel.
#pragma once

#include "pt_render_kernel.h"
#include "pt_rays_inst.h"

template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK, pt_rays_waves(MODE)) pt_rays_kernel(PtRaysArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    constexpr bool MESHES = !(MODE == PT_MODE_FLAT_NOMESH || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_KD_NOMESH);
    extern __shared__ uint32_t pt_lds[];
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

    // items are handed out one at a time from interleaved queues (pt_aov_kernel, pt_render_simple_kernel): item idx * N + q from queue q
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
        if (mine) {
            const double* o = a0.origins + 3 * i;
            const double* d = a0.directions + 3 * i;
            ray.o = pt_v3(o[0], o[1], o[2]);
            ray.d = pt_v3(d[0], d[1], d[2]);
        }
        const bool traced = mine && pt_rays_traced(ray);
        if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
        PtHit hit;
        hit.t = INFINITY; hit.node = PT_NO_HIT; hit.sub = 0;
        if (__any(traced)) pt_trace_wave<MODE, false>(a, ray, traced, any, hit, stk, pt_lds, &cnt);
        if (!mine) continue;  // (a lane past n: nothing to write)

        const bool ok = traced && hit.node != PT_NO_HIT;
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
static hipError_t pt_rays_launch(const PtRaysArgs& a, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = (size_t)a.r.stack_lds_cap * PT_BLOCK * 4;  // the traversal stack area alone
    return pt_launch_kernel_args<&pt_rays_kernel<MODE>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}
