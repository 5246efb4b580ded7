// One traversal mode's instantiations of pt_lens_kernel - the film's sampling kernel behind a lens (pt_film_add_lens, include/portrayer_hip.h) -
// and their launcher. Compiled once per mode, -DPT_INST_MODE=1..9 (Makefile: pt_lens_m<mode>.o), beside the film's objects and through the same check / repair
// of the assembly.
//
// Every pixel of a slice gets its NEXT samples exactly as pt_film_kernel (pt_film.h) gives them - the same work item (one wavefront = 64 / K pixel slots of an
// 8x8 tile x K lanes per pixel, pt_film_item_slot), the same staging writes for pt_film_fold_kernel behind it - and only the primary ray of a sample differs:
// it is the lens contract's (pt_lens.h), made in registers where the sample starts. No ray is ever in memory.
//
// Nothing of the shading is new: this is pt_film_kernel's frame - persistent wavefronts, one item at a time from 16 interleaved queues, the argument block
// re-read through the kernarg segment, 3 waves per SIMD, LDS as pt_render_lds_bytes lays it out - around pt_source_advance with PtLensSource
// (pt_lens_inst.h). The lens' four fields are read through the kernarg segment inside the policy: scalar loads, the model's branch is wave-uniform.
#include "pt_film.h"
#include "pt_lens_inst.h"

#ifndef PT_INST_MODE
#error "compile with -DPT_INST_MODE=<PT_MODE_*>"
#endif
#define PT_INST_CAT2(a, b) a##b
#define PT_INST_CAT(a, b) PT_INST_CAT2(a, b)

// The argument block seen again through the kernarg segment (pt_film_args_again)
PT_HD const PtLensArgs& pt_lens_args_again(const PtLensArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) PtLensArgs* ka = (const __attribute__((address_space(4))) PtLensArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(const PtLensArgs*)ka;
#else
    return a;
#endif
}

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_lens_waves(MODE)) pt_lens_kernel(PtLensArgs a0) {
    constexpr bool HIER = MODE == PT_MODE_HIER || MODE == PT_MODE_HIER_NOMESH || MODE == PT_MODE_HIER_MESH;
    extern __shared__ uint32_t pt_lds[];
    const PtRenderArgs& a = a0.f.r;
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
        uint32_t j, x, y;
        const uint32_t slot = pt_film_item_slot(w, lane, a0.f.k_log2, &j);
        const bool mine = pt_slot_to_pixel(a, slot, &x, &y) && j < a0.f.launch_samples;  // (inside the slice, so inside the image: count has a word for it)
        uint32_t s = 0;
        if (mine) s = a0.f.count[(size_t)y * a.width + x] + j;  // the pixel's next samples, in lane order
        L.item = s;
        L.x = mine ? x : 0u;
        L.y = mine ? y : 0u;
        L.ray.o = L.ray.d = pt_v3(0.0, 0.0, 0.0);
        L.stage = mine ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
        L.has_ray = false;
        for (;;) {
            const bool active = L.stage != PT_ST_DONE;
            if (!__any(active)) break;
            // what the interpreter and this pass's walk need of the arguments is fetched now, not kept from the top of the kernel on (pt_render_kernel)
            const PtLensArgs& aa = pt_lens_args_again(a0);
            const PtRenderArgs& a = aa.f.r;
            PtLensSource src;
            src.lens = &aa.lens;
            if (active) pt_source_advance<TEX, HIER, PARK, PtLensSource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its place in the staging buffer, worked out again
        // from the item (slot < n_slots because w < n_items = own tiles x K; j < launch_samples <= lw)
        if (mine) {
            const PtFilmArgs& aa = pt_lens_args_again(a0).f;
            uint32_t j2;
            const uint32_t slot2 = pt_film_item_slot(w, lane, aa.k_log2, &j2);
            const PtVec3 value = fr.l3(PT_L_VALUE);
            double* o = aa.staging + 3 * ((size_t)slot2 * aa.lw + j2);
            o[0] = value.x; o[1] = value.y; o[2] = value.z;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_lens_launch(const PtLensArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = pt_render_lds_bytes(a.f.r.stack_lds_cap, tex, park ? 1 : 0);
    if (tex) {
        if (park) return pt_launch_kernel_args<&pt_lens_kernel<MODE, true, 1>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
        return pt_launch_kernel_args<&pt_lens_kernel<MODE, true, 0>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
    }
    if (park) return pt_launch_kernel_args<&pt_lens_kernel<MODE, false, 1>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<&pt_lens_kernel<MODE, false, 0>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
}

hipError_t PT_INST_CAT(pt_lens_launch_mode_, PT_INST_MODE)(const PtLensArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch) {
    return pt_lens_launch<PT_INST_MODE>(a, tex, park, n_cu, stream, grid, launch);
}
