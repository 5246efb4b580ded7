// The film's sampling kernel (pt_film_add, include/portrayer_hip.h): every pixel of a slice gets its NEXT samples - count[p] .. count[p] + m - 1, m <= lw -
// each taken exactly as pt_render takes that sample of that pixel, and written, one 24-byte value per (pixel slot, place in the launch), to a staging buffer
// that pt_film_fold_kernel (pt_film.hip) folds into the film behind this kernel on the same stream.
//
// Work item: one wavefront = 64 / K consecutive pixel slots of one 8x8 tile of the slice (pt_slot_to_pixel's order: rows of the tile) x K lanes per pixel,
// K = the next power of two >= m: a pixel's samples sit in neighbouring lanes, lanes j >= m idle. Item w = local tile * K + part.
//
// Nothing of the shading is new: this is pt_radiance_kernel's frame (pt_radiance.h) - persistent wavefronts, one item at a time from 16 interleaved queues, the
// argument block re-read through the kernarg segment, 3 waves per SIMD, LDS as pt_render_lds_bytes lays it out - around pt_source_advance with PtFilmSource
// (pt_film_inst.h): the primary ray from the camera through the jittered pixel, the background at the pixel, stream y * width + x, and the sample index per
// LANE, carried in L.item. The generator is counter-based, so sample s of a pixel is what it is in a render of any length, whatever shares its wavefront.
#pragma once

#include "pt_radiance.h"
#include "pt_film_inst.h"

// The argument block seen again through the kernarg segment (pt_radiance_args_again)
PT_HD const PtFilmArgs& pt_film_args_again(const PtFilmArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) PtFilmArgs* ka = (const __attribute__((address_space(4))) PtFilmArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(const PtFilmArgs*)ka;
#else
    return a;
#endif
}

// Item w, lane -> the lane's pixel slot and its place j in the launch (K = 1 << kl lanes per pixel)
PT_HD uint32_t pt_film_item_slot(uint32_t w, uint32_t lane, uint32_t kl, uint32_t* j) {
    const uint32_t tile_local = w >> kl, part = w & ((1u << kl) - 1u);
    *j = lane & ((1u << kl) - 1u);
    return (tile_local << 6) | ((part << (6u - kl)) + (lane >> kl));
}

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_film_waves(MODE)) pt_film_kernel(PtFilmArgs a0) {
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
        uint32_t j, x, y;
        const uint32_t slot = pt_film_item_slot(w, lane, a0.k_log2, &j);
        const bool mine = pt_slot_to_pixel(a, slot, &x, &y) && j < a0.launch_samples;  // (inside the slice, so inside the image: count has a word for it)
        uint32_t s = 0;
        if (mine) s = a0.count[(size_t)y * a.width + x] + j;  // the pixel's next samples, in lane order
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
            const PtFilmArgs& aa = pt_film_args_again(a0);
            const PtRenderArgs& a = aa.r;
            PtFilmSource src;
            if (active) pt_source_advance<TEX, HIER, PARK, PtFilmSource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its place in the staging buffer, worked out again
        // from the item (slot < n_slots because w < n_items = own tiles x K; j < launch_samples <= lw)
        if (mine) {
            const PtFilmArgs& aa = pt_film_args_again(a0);
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
static hipError_t pt_film_launch(const PtFilmArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = pt_render_lds_bytes(a.r.stack_lds_cap, tex, park ? 1 : 0);
    if (tex) {
        if (park) return pt_launch_kernel_args<&pt_film_kernel<MODE, true, 1>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
        return pt_launch_kernel_args<&pt_film_kernel<MODE, true, 0>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
    }
    if (park) return pt_launch_kernel_args<&pt_film_kernel<MODE, false, 1>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<&pt_film_kernel<MODE, false, 0>>(lds, a, a.r.n_items, a.r.grid_share, n_cu, stream, grid_out, launch);
}
