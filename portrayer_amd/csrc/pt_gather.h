// The gather pass's kernel (pt_gather, include/portrayer_hip.h): per point, the sum of `samples` shaded radiance samples along the rays the
// ambient-occlusion contract gives that point (pt_ao.h, steps 1 to 8) - sample k of point q being, to the bit, what pt_radiance answers for that ray with the
// call's background and the generator's stream (seed, q * S + k, pass). No ray and no per-ray colour is ever in memory: 48 bytes per point in, 25 out.
//
// Work item: one wavefront = 64 / S consecutive points x S samples, lane l = (point l / S, sample l % S) - pt_ao_kernel's point-major layout, a point's rays
// starting together. A lane makes its ray in registers when the item starts; lanes of invalid points (pt_ao_valid), lanes past n and rays pt_radiance would not
// trace (pt_rays_traced: the origin can leave the range through a huge bias) take no part in a walk, the last kind leaving the background in their own column.
//
// Nothing of the shading is new: the kernel's frame is the shading passes' (pt_shade_frame.h holds it for the film's kernels, this kernel keeps its
// own copy because on the shared frame two of its instantiations spill differently) around pt_source_advance with PtGatherSource
// (pt_gather_inst.h). When every lane is PT_ST_DONE each lane's sample sits in its own LDS column (PT_L_VALUE); behind a wavefront barrier the first lane of a
// point's group adds the group's S columns from (0, 0, 0) in ascending k and writes the point's 24 bytes - pt_ao_kernel's pattern for `bent`, and the render
// kernels' for a chunk's sum - so the pass needs no LDS beyond the frame's.
#pragma once

#include "pt_radiance.h"
#include "pt_gather_inst.h"

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_gather_waves(MODE)) pt_gather_kernel(PtGatherArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a0.r;
    const uint32_t lane_global = blockIdx.x * PT_BLOCK + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    PtStackSpill stk;
    stk.base = pt_lds + threadIdx.x;
    stk.cap = a.stack_lds_cap;
    stk.total = a.scene.stack_cap;
    stk.gbase = a.stack_spill + lane_global;
    stk.gstride = a.n_lanes;
    stk.overflow = a.overflow_flag;
    PtFrameRef fr;
    fr.lds = reinterpret_cast<double*>(pt_lds + (size_t)a.stack_lds_cap * PT_BLOCK) + threadIdx.x;
    fr.park = fr.lds + (size_t)PT_LDS_FRAME_F64 * PT_FRAME_STRIDE;
    fr.spill = a.spill + (size_t)lane_global * (PT_SPILL_DEPTHS * PT_SPILL_STRIDE);
    fr.n_lanes = a.n_lanes;
    PtCounters cnt;  // (the walks and the interpreter take a pointer; nothing is counted)
    PtLane L;
    L.stage = PT_ST_DONE; L.has_ray = false; L.ray_any = false;
    L.item = 0; L.x = L.y = 0; L.light = L.draw = L.draw0 = L.occluded = 0; L.depth = 0; L.lo = 0;
    L.ray.o = L.ray.d = pt_v3(0.0, 0.0, 0.0);
    L.offer = false; L.base = 0; L.owner = 0; L.fork_seq = 0; L.ticket = 0; L.wait_ticket = 0;
    PtHit hit;
    hit.t = INFINITY; hit.node = PT_NO_HIT; hit.sub = 0;

    // items are handed out one at a time from interleaved queues (pt_radiance_kernel): item idx * N + q from queue q
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
        const unsigned sh = a0.log2_samples;
        const unsigned k = lane & (a0.samples - 1u);
        const uint64_t p = ((uint64_t)w << (6u - sh)) + (lane >> sh);  // (w < n_items <= 2^24)
        const bool mine = p < a0.n;
        PtRay ray;
        ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);
        const bool valid = mine && pt_gather_ray(a0, p, k, &ray);  // (the same answer in every lane of a point's group)
        const bool traced = valid && pt_rays_traced(ray);
        // not traced: pt_radiance's answer for such a ray is its background colour; it waits in the lane's column like a finished sample
        if (valid && !traced) fr.set_l3(PT_L_VALUE, pt_v3(a0.background[0], a0.background[1], a0.background[2]));
        if (!traced) ray.o = ray.d = pt_v3(0.0, 0.0, 0.0);  // what an idle lane of the render kernels holds: no NaN reaches the walk's arithmetic
        L.item = w;
        L.x = traced ? (uint32_t)p : 0u;  // the point's index in the call and the sample: what the source policy works the stream out from
        L.y = traced ? k : 0u;
        L.ray = ray;
        L.stage = traced ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
        L.has_ray = false;
        for (;;) {
            const bool active = L.stage != PT_ST_DONE;
            if (!__any(active)) break;
            // what the interpreter and this pass's walk need of the arguments is fetched now, not kept from the top of the kernel on (pt_render_kernel)
            const PtGatherArgs& aa = pt_args_again(a0);
            const PtRenderArgs& a = aa.r;
            PtGatherSource src;
            src.first_index = aa.set.first_index; src.samples = aa.samples; src.pass = aa.set.pass;
            src.bg = pt_v3(aa.background[0], aa.background[1], aa.background[2]);
            if (active) pt_source_advance<TEX, HIER, PARK, PtGatherSource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // every lane's finished sample is in its own LDS column; the group's first lane reads its neighbours': same wavefront, so a wavefront barrier between
        // the last interpreter step and the reads (pt_ao_kernel's bent normal)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // One lane per point writes; its group is lanes lane .. lane + S - 1, inside the wavefront. The point, and whether it is valid, are worked out again from
        // the item (pt_render_kernel's w_again: the empty asm keeps the compiler from carrying the first computation through the walks in registers).
        unsigned w_again = w;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(w_again));
#endif
        const PtGatherArgs& ab = pt_args_again(a0);
        const uint64_t p_again = ((uint64_t)w_again << (6u - ab.log2_samples)) + (lane >> ab.log2_samples);
        if (p_again < ab.n && (lane & (ab.samples - 1u)) == 0u) {
            const double* P = ab.positions + 3 * (size_t)p_again;
            const double* N = ab.normals + 3 * (size_t)p_again;
            const bool valid_again = pt_ao_valid(pt_v3(P[0], P[1], P[2]), pt_v3(N[0], N[1], N[2]));
            PtVec3 sum = pt_v3(0.0, 0.0, 0.0);
            if (valid_again)
                for (unsigned j = 0; j < ab.samples && j < 64u; j++) {  // (bounded by a constant as well)
                    const double* o = fr.lds + j;
                    sum = sum + pt_v3(o[(PT_L_VALUE + 0) * PT_FRAME_STRIDE], o[(PT_L_VALUE + 1) * PT_FRAME_STRIDE], o[(PT_L_VALUE + 2) * PT_FRAME_STRIDE]);
                }
            if (ab.sum) { double* o = ab.sum + 3 * (size_t)p_again; o[0] = sum.x; o[1] = sum.y; o[2] = sum.z; }
            if (ab.valid) ab.valid[p_again] = valid_again ? 1 : 0;
        }
        __builtin_amdgcn_wave_barrier();  // the columns are free for the next item
    }
}

// What pt_shade_launch (pt_shade_frame.h) asks of a pass
struct PtGatherPass {
    using Args = PtGatherArgs;
    static PT_HD const PtRenderArgs& render(const PtGatherArgs& a0) { return a0.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_gather_kernel<MODE, TEX, PARK>; }
};
