// The film's list-driven sampling kernel (pt_film_add_map, include/portrayer_hip.h): pixels of a slice want DIFFERENT numbers of samples, so the
// work is not laid out per pixel but per sample. The plan kernels (pt_film_map.hip) write one u32 per sample of the round - slot * PT_FILM_LW + j, in
// ascending (slot, j) order, so a pixel's samples and a tile's pixels stay neighbours - and the list's length to a device word; wavefront w takes entries
// 64 w .. 64 w + 63. Every lane below the list's length carries a ray: none idles because its pixel wanted fewer samples than its neighbour.
//
// The frame is the shading passes' (pt_shade_frame.h) and the source the film's (PtFilmSource): the sample index per lane in L.item = count[p] + j, the value to
// staging[entry]. The host does not know the list's length (a device map): it sizes the grid from its upper bound, the kernel reads the length and wavefronts
// that find nothing leave.
#pragma once

#include "pt_film.h"
#include "pt_film_map_inst.h"

template <int MODE, bool TEX, int PARK>
__global__ void pt_film_map_kernel(PtFilmMapArgs a0);

// The pass's policy for pt_shade_frame
struct PtFilmMapPass {
    using Args = PtFilmMapArgs;
    using Source = PtFilmSource;
    struct Item { uint32_t n_list; bool mine; };
    static PT_HD const PtRenderArgs& render(const PtFilmMapArgs& a0) { return a0.f.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_film_map_kernel<MODE, TEX, PARK>; }

    // The number of items is the DEVICE's: the list's length in wavefronts, never more than the host's bound the grid and the buffers were sized for.
    static __device__ __forceinline__ uint32_t bound(const PtFilmMapArgs& a0, const PtRenderArgs& a, Item& it) {
        it.n_list = (uint32_t)__builtin_amdgcn_readfirstlane((int)*a0.n_list);  // (one address for the wavefront: kept where the loop's conditions are scalar)
        const uint32_t n_waves = (it.n_list >> 6) + ((it.n_list & 63u) ? 1u : 0u);
        return n_waves < a.n_items ? n_waves : a.n_items;
    }
    static __device__ __forceinline__ void begin(const PtFilmMapArgs& a0, const PtRenderArgs& a, unsigned w, unsigned lane, Item& it, PtLane& L, const PtFrameRef&) {
        const uint32_t e = (w << 6) + lane;  // (w < n_items <= n_slots * lw / 64: no wrap)
        bool mine = e < it.n_list;
        uint32_t x = 0, y = 0, s = 0;
        if (mine) {
            const uint32_t entry = a0.list[e];
            mine = pt_slot_to_pixel(a, entry >> PT_FILM_MAP_LW_LOG2, &x, &y);  // (the plan lists pixels of the slice only: count has a word for them)
            if (mine) s = a0.f.count[(size_t)y * a.width + x] + (entry & ((1u << PT_FILM_MAP_LW_LOG2) - 1u));  // the pixel's next samples, in list order
        }
        it.mine = mine;
        L.item = s;
        L.x = mine ? x : 0u;
        L.y = mine ? y : 0u;
        L.ray.o = L.ray.d = pt_v3(0.0, 0.0, 0.0);
        L.stage = mine ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
        L.has_ray = false;
    }
    static __device__ __forceinline__ void source(const PtFilmMapArgs&, PtFilmSource&) {}
    // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its place in the staging buffer: its entry, read
    // again (entry < n_slots * lw: slot < n_slots, j < lw)
    static __device__ __forceinline__ void finish(const PtFilmMapArgs& a0, unsigned w, unsigned lane, const Item& it, const PtLane&, const PtFrameRef& fr) {
        if (it.mine) {
            const PtFilmMapArgs& aa = pt_args_again(a0);
            const uint32_t entry = aa.list[(w << 6) + lane];
            const PtVec3 value = fr.l3(PT_L_VALUE);
            double* o = aa.f.staging + 3 * (size_t)entry;
            o[0] = value.x; o[1] = value.y; o[2] = value.z;
        }
    }
};

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_film_waves(MODE)) pt_film_map_kernel(PtFilmMapArgs a0) {
    pt_shade_frame<MODE, TEX, PARK, PtFilmMapPass>(a0);
}
