// The film's sampling kernel (pt_film_add, include/portrayer_hip.h): every pixel of a slice gets its NEXT samples - count[p] .. count[p] + m - 1, m <= lw -
// each taken exactly as pt_render takes that sample of that pixel, and written, one 24-byte value per (pixel slot, place in the launch), to a staging buffer
// that pt_film_fold_kernel (pt_film.hip) folds into the film behind this kernel on the same stream.
//
// Work item: one wavefront = 64 / K consecutive pixel slots of one 8x8 tile of the slice (pt_slot_to_pixel's order: rows of the tile) x K lanes per pixel,
// K = the next power of two >= m: a pixel's samples sit in neighbouring lanes, lanes j >= m idle. Item w = local tile * K + part.
//
// Nothing of the shading is new: the shading passes' frame (pt_shade_frame.h) around pt_source_advance with PtFilmSource (pt_film_inst.h): the primary ray
// from the camera through the jittered pixel, the background at the pixel, stream y * width + x, and the sample index per LANE, carried in L.item. The
// generator is counter-based, so sample s of a pixel is what it is in a render of any length, whatever shares its wavefront.
#pragma once

#include "pt_radiance.h"
#include "pt_film_inst.h"

// Item w, lane -> the lane's pixel slot and its place j in the launch (K = 1 << kl lanes per pixel)
PT_HD uint32_t pt_film_item_slot(uint32_t w, uint32_t lane, uint32_t kl, uint32_t* j) {
    const uint32_t tile_local = w >> kl, part = w & ((1u << kl) - 1u);
    *j = lane & ((1u << kl) - 1u);
    return (tile_local << 6) | ((part << (6u - kl)) + (lane >> kl));
}

template <int MODE, bool TEX, int PARK>
__global__ void pt_film_kernel(PtFilmArgs a0);

// The pass's policy for pt_shade_frame. begin and finish take a PtFilmArgs, which may be the start of a longer block (offsetof(.., f) == 0).
struct PtFilmPass : PtShadeItems {
    using Args = PtFilmArgs;
    using Source = PtFilmSource;
    struct Item { bool mine; };
    static PT_HD const PtRenderArgs& render(const PtFilmArgs& a0) { return a0.r; }
    template <int MODE, bool TEX, int PARK>
    static constexpr auto kernel() { return &pt_film_kernel<MODE, TEX, PARK>; }

    static __device__ __forceinline__ void begin(const PtFilmArgs& a0, const PtRenderArgs& a, unsigned w, unsigned lane, Item& it, PtLane& L, const PtFrameRef&) {
        uint32_t j, x, y;
        const uint32_t slot = pt_film_item_slot(w, lane, a0.k_log2, &j);
        const bool mine = pt_slot_to_pixel(a, slot, &x, &y) && j < a0.launch_samples;  // (inside the slice, so inside the image: count has a word for it)
        uint32_t s = 0;
        if (mine) s = a0.count[(size_t)y * a.width + x] + j;  // the pixel's next samples, in lane order
        it.mine = mine;
        L.item = s;
        L.x = mine ? x : 0u;
        L.y = mine ? y : 0u;
        L.ray.o = L.ray.d = pt_v3(0.0, 0.0, 0.0);
        L.stage = mine ? PT_ST_NEW_SAMPLE : PT_ST_DONE;
        L.has_ray = false;
    }
    static __device__ __forceinline__ void source(const PtFilmArgs&, PtFilmSource&) {}
    // the lane's own finished sample, out of its own LDS column (same lane: program order suffices), to its place in the staging buffer, worked out again
    // from the item (slot < n_slots because w < n_items = own tiles x K; j < launch_samples <= lw)
    static __device__ __forceinline__ void finish(const PtFilmArgs& a0, unsigned w, unsigned lane, const Item& it, const PtLane&, const PtFrameRef& fr) {
        if (it.mine) {
            const PtFilmArgs& aa = pt_args_again(a0);
            uint32_t j2;
            const uint32_t slot2 = pt_film_item_slot(w, lane, aa.k_log2, &j2);
            const PtVec3 value = fr.l3(PT_L_VALUE);
            double* o = aa.staging + 3 * ((size_t)slot2 * aa.lw + j2);
            o[0] = value.x; o[1] = value.y; o[2] = value.z;
        }
    }
};

template <int MODE, bool TEX, int PARK>
__global__ void __launch_bounds__(PT_BLOCK, pt_film_waves(MODE)) pt_film_kernel(PtFilmArgs a0) {
    pt_shade_frame<MODE, TEX, PARK, PtFilmPass>(a0);
}
