// The film's list-driven sampling kernel (pt_film_add_map, include/portrayer_hip.h): pixels of a slice want DIFFERENT numbers of samples, so the
// work is not laid out per pixel but per sample. The plan kernels (pt_film_map.hip) write one u32 per sample of the round - slot * PT_FILM_LW + j, in
// ascending (slot, j) order, so a pixel's samples and a tile's pixels stay neighbours - and the list's length to a device word; wavefront w takes entries
// 64 w .. 64 w + 63. Every lane below the list's length carries a ray: none idles because its pixel wanted fewer samples than its neighbour.
//
// The frame is pt_film_kernel's (pt_film.h), unchanged: persistent wavefronts, items from 16 interleaved queues, the argument block re-read through the kernarg
// segment, 3 waves per SIMD, PtFilmSource around pt_source_advance, the sample index per lane in L.item = count[p] + j, the value to staging[entry]. The host
// does not know the list's length (a device map): it sizes the grid from its upper bound, the kernel reads the length and wavefronts that find nothing leave.
#pragma once

#include "pt_film.h"
#include "pt_film_map_inst.h"

PT_HD const PtFilmMapArgs& pt_film_map_args_again(const PtFilmMapArgs& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) PtFilmMapArgs* ka = (const __attribute__((address_space(4))) PtFilmMapArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(const PtFilmMapArgs*)ka;
#else
    return a;
#endif
}

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_film_waves(MODE)) pt_film_map_kernel(PtFilmMapArgs a0) {
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

    // items are handed out one at a time from interleaved queues (pt_film_kernel): item idx * N + q from queue q. The number of items is the DEVICE's:
    // the list's length in wavefronts, never more than the host's bound the grid and the buffers were sized for.
    unsigned q_next = blockIdx.x % a.fine_queues, q_end = 0;
    for (;;) {
        unsigned w;
        uint32_t n_list;
        for (;;) {
            unsigned idx = 0;
            if (lane == 0) idx = atomicAdd(a.work_queues + q_next * PT_QUEUE_STRIDE, 1u);
            idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
            const unsigned long long pos = (unsigned long long)idx * a.fine_queues + q_next;
            n_list = (uint32_t)__builtin_amdgcn_readfirstlane((int)*a0.n_list);  // (one address for the wavefront: kept where the loop's conditions are scalar)
            const uint32_t n_waves = (n_list >> 6) + ((n_list & 63u) ? 1u : 0u);
            if (pos < (n_waves < a.n_items ? n_waves : a.n_items)) { w = (unsigned)pos; q_end = 0; break; }
            q_next = q_next + 1u == a.fine_queues ? 0u : q_next + 1u;
            if (++q_end == a.fine_queues) { w = 0xFFFFFFFFu; break; }
        }
        if (w == 0xFFFFFFFFu) break;
        const uint32_t e = (w << 6) + lane;  // (w < n_items <= n_slots * lw / 64: no wrap)
        bool mine = e < n_list;
        uint32_t x = 0, y = 0, s = 0;
        if (mine) {
            const uint32_t entry = a0.list[e];
            mine = pt_slot_to_pixel(a, entry >> PT_FILM_MAP_LW_LOG2, &x, &y);  // (the plan lists pixels of the slice only: count has a word for them)
            if (mine) s = a0.f.count[(size_t)y * a.width + x] + (entry & ((1u << PT_FILM_MAP_LW_LOG2) - 1u));  // the pixel's next samples, in list order
        }
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
            const PtFilmMapArgs& aa = pt_film_map_args_again(a0);
            const PtRenderArgs& a = aa.f.r;
            PtFilmSource src;
            if (active) pt_source_advance<TEX, HIER, PARK, PtFilmSource>(a, L, hit, fr, &cnt, 0u, src);
            const bool tracing = L.stage != PT_ST_DONE && L.has_ray;
            if (__any(tracing)) pt_trace_wave<MODE, false>(a, L.ray, tracing, L.ray_any, hit, stk, pt_lds, &cnt);
        }
        // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its place in the staging buffer: its entry, read
        // again (entry < n_slots * lw: slot < n_slots, j < lw)
        if (mine) {
            const PtFilmMapArgs& aa = pt_film_map_args_again(a0);
            const uint32_t entry = aa.list[(w << 6) + lane];
            const PtVec3 value = fr.l3(PT_L_VALUE);
            double* o = aa.f.staging + 3 * (size_t)entry;
            o[0] = value.x; o[1] = value.y; o[2] = value.z;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Launch (or, with launch = false, only size) the pass: the grid is what is resident, by the render kernels' launcher (pt_launch_kernel_args).
template <int MODE>
static hipError_t pt_film_map_launch(const PtFilmMapArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid_out, bool launch) {
    const size_t lds = pt_render_lds_bytes(a.f.r.stack_lds_cap, tex, park ? 1 : 0);
    if (tex) {
        if (park) return pt_launch_kernel_args<&pt_film_map_kernel<MODE, true, 1>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
        return pt_launch_kernel_args<&pt_film_map_kernel<MODE, true, 0>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
    }
    if (park) return pt_launch_kernel_args<&pt_film_map_kernel<MODE, false, 1>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
    return pt_launch_kernel_args<&pt_film_map_kernel<MODE, false, 0>>(lds, a, a.f.r.n_items, a.f.r.grid_share, n_cu, stream, grid_out, launch);
}
