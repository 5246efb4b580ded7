// The frame of the shading passes: what pt_radiance_kernel, pt_film_kernel, pt_film_map_kernel, pt_lens_kernel, pt_gather_kernel and
// pt_probe_kernel share. pt_film_kernel, pt_film_map_kernel and pt_lens_kernel are shells that call pt_shade_frame with their PASS policy; pt_radiance_kernel,
// pt_gather_kernel and pt_probe_kernel still carry the same text themselves, because moved behind the policy calls their begin (the pt_rays_traced test) is
// simplified once more before it meets the walks and some of their instantiations then spill differently (profiles/r17/notes.md). All six share pt_args_again
// and the launcher below.
//
// The frame: persistent wavefronts, 3 waves per SIMD; LDS of a block as in pt_render_kernel - the traversal stack area, the hit frame per lane, and (PARK = 1)
// the youngest parked recursion frame per lane, as pt_render_lds_bytes lays it out; older frames in the lane's own 128-byte lines in HBM (PtRenderArgs::spill).
// Items are handed out one at a time from 16 interleaved queues. Per item every lane runs the interpreter with the pass's source (pt_source_advance,
// pt_radiance.h) to the end of its sample, all 64 lanes meeting in the one pt_trace_wave<MODE> per step whatever kind of ray each carries; the argument block is
// re-read through the kernarg segment per step, so that it is not carried across the walks in registers. No counting variant, no fork / join, no occluder table.
//
// A PASS policy carries what differs:
//   Args, Source      the kernel's argument block, which starts with a PtRenderArgs or with a block that does, and the SRC of pt_source_advance
//   Item              what begin (and bound) leave for finish
//   render(a0)        the PtRenderArgs in the block
//   kernel<MODE, TEX, PARK>()   the pass's __global__ shell, for the launcher
//   bound(a0, a, it)  the number of items the queues hand out
//   begin(a0, a, w, lane, it, L, fr)   item and lane -> the lane's ray, L.item, L.x, L.y and its stage; what an untraced ray answers
//   source(aa, src)   the source filled from the re-read arguments
//   finish(a0, w, lane, it, L, fr)     what every lane does with the finished samples, each in its own LDS column (PT_L_VALUE)
// The body is ONE function and the seams are these calls, all inlined: cut into helpers (the set-up, the pop, the inner loop) the same text spills more
// registers in every instantiation (profiles/r17/notes.md).
#pragma once

#include "pt_render_kernel.h"

// The argument block seen again through the kernarg segment (pt_args_again, pt_render_simple.h): what a pass needs of it is fetched where it is used.
template <class ARGS>
PT_HD const ARGS& pt_args_again(const ARGS& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) ARGS* ka = (const __attribute__((address_space(4))) ARGS*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(const ARGS*)ka;
#else
    return a;
#endif
}

// The interpreter with a source (pt_radiance.h)
template <bool TEX, bool HIER, int PARK, class SRC>
PT_HD void pt_source_advance(const PtRenderArgs& a, PtLane& L, const PtHit& hit, const PtFrameRef& fr, PtCounters* cnt, uint32_t pre, const SRC& src);

// bound for the passes whose host knows the number of items
struct PtShadeItems {
    template <class ARGS, class ITEM>
    static PT_HD uint32_t bound(const ARGS&, const PtRenderArgs& a, ITEM&) { return a.n_items; }
};

template <int MODE, bool TEX, int PARK, class PASS>
__device__ __forceinline__ void pt_shade_frame(const typename PASS::Args& a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = PASS::render(a0);
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

    // items are handed out one at a time from interleaved queues (pt_rays_kernel, pt_render_kernel): item idx * N + q from queue q
    unsigned q_next = blockIdx.x % a.fine_queues, q_end = 0;
    for (;;) {
        unsigned w;
        typename PASS::Item it;
        for (;;) {
            unsigned idx = 0;
            if (lane == 0) idx = atomicAdd(a.work_queues + q_next * PT_QUEUE_STRIDE, 1u);
            idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
            const unsigned long long pos = (unsigned long long)idx * a.fine_queues + q_next;
            if (pos < PASS::bound(a0, a, it)) { w = (unsigned)pos; q_end = 0; break; }
            q_next = q_next + 1u == a.fine_queues ? 0u : q_next + 1u;
            if (++q_end == a.fine_queues) { w = 0xFFFFFFFFu; break; }
        }
        if (w == 0xFFFFFFFFu) break;
        PASS::begin(a0, a, w, lane, it, L, fr);
        for (;;) {
            const bool active = L.stage != PT_ST_DONE;
            if (!__any(active)) break;
            // what the interpreter and this pass's walk need of the arguments is fetched now, not kept from the top of the kernel on (pt_render_kernel)
            const typename PASS::Args& aa = pt_args_again(a0);
            const PtRenderArgs& a = PASS::render(aa);
            typename PASS::Source src;
            PASS::source(aa, src);
            if (active) pt_source_advance<TEX, HIER, PARK, typename PASS::Source>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        PASS::finish(a0, w, lane, it, L, fr);
        __builtin_amdgcn_wave_barrier();  // the columns are free for the next item
    }
}

// Launch (or, with launch = false, only size) a pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
// tex, park: the scene has a material map; it has a dielectric (the youngest parked frame in LDS).
template <int MODE, class PASS>
static hipError_t pt_shade_launch(const typename PASS::Args& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const PtRenderArgs& r = PASS::render(a);
    const size_t lds = pt_render_lds_bytes(r.stack_lds_cap, tex, park ? 1 : 0);
    if (tex) {
        if (park) return pt_launch_kernel_args<PASS::template kernel<MODE, true, 1>()>(lds, a, r.n_items, r.grid_share, n_cu, stream, grid_out, launch);
        return pt_launch_kernel_args<PASS::template kernel<MODE, true, 0>()>(lds, a, r.n_items, r.grid_share, n_cu, stream, grid_out, launch);
    }
    if (park) return pt_launch_kernel_args<PASS::template kernel<MODE, false, 1>()>(lds, a, r.n_items, r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<PASS::template kernel<MODE, false, 0>()>(lds, a, r.n_items, r.grid_share, n_cu, stream, grid_out, launch);
}
