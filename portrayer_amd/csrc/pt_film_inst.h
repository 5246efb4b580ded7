// The film (pt_film_*, include/portrayer_hip.h): the argument block of its sampling kernel, the source policy that makes the interpreter
// (pt_source_advance, pt_radiance.h) take a RENDER's samples, the two functions that hold the summation contract for a running sum, and the launchers -
// one per traversal mode for the sampling kernel, each in its own object (pt_film_inst.hip compiled with -DPT_INST_MODE=<mode>), and the fold and resolve
// kernels' (pt_film.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_radiance_inst.h"

// Most samples per pixel one launch of the sampling kernel takes (a longer pt_film_add is several launches, each followed by its fold): the staging buffer
// holds this many 24-byte samples per pixel slot of the slice. 8 or 64 (PORTRAYER_FILM_LW, measurements): profiles/film/notes.md.
#define PT_FILM_LW 8

struct PtFilmArgs {
    PtRenderArgs r;             // scene, camera, background, image size, slice (x0 .. y1, tile_rank 0 of 1, n_slots), seed, jitter_mode; recursion frames, stack areas,
                                // work queues, overflow flag; n_items = own tiles x K. FIRST: the kernel re-reads the block through the kernarg segment
    const uint32_t* count;      // width x height: samples every pixel holds BEFORE this launch (its fold adds launch_samples behind the kernel)
    double* staging;            // n_slots x lw x 3: sample j of this launch of pixel slot p at (p * lw + j)
    uint32_t launch_samples;    // samples per pixel of this launch, 1 .. lw
    uint32_t k_log2;            // K = 1 << k_log2 = the next power of two >= launch_samples: lanes of a wavefront per pixel
    uint32_t lw;                // stride of a pixel slot in `staging`, in samples
};
static_assert(offsetof(PtFilmArgs, r) == 0, "the kernel reads PtRenderArgs at the start of its argument block");

// The film's source (SRC of pt_source_advance / pt_source_light_position): what pt_lane_advance (pt_shade.h) reads of the camera, the pixel and the item, with
// the sample index per LANE. The lane carries its pixel in L.x, L.y and its absolute sample index (the pixel's count + its place in the launch) in L.item, a
// field the interpreter and the walks never read or write (pt_source_advance reads the lane's sample through src.sample alone).
struct PtFilmSource {
    PT_HD uint32_t sample(const PtRenderArgs&, const PtLane& L) const { return L.item; }
    PT_HD uint64_t stream(const PtRenderArgs& a, const PtLane& L) const { return (uint64_t)L.y * a.width + L.x; }
    PT_HD PtVec3 background(const PtRenderArgs& a, const PtLane& L) const { return pt_background(a, L.x, L.y); }
    PT_HD PtRay primary(const PtRenderArgs& a, const PtLane& L) const {  // pt_lane_advance's PT_ST_NEW_SAMPLE
        double jx = 0.5, jy = 0.5;
        if (a.jitter_mode == PT_JITTER_RNG) {  // render.rs:38-39: x drawn before y
            const uint32_t s = L.item;
            uint64_t pixel = (uint64_t)L.y * a.width + L.x;
            jx = pt_rng_f64(a.seed, pixel, s, 0);
            jy = pt_rng_f64(a.seed, pixel, s, 1);
        }
        return pt_camera_ray(a.cam, (double)L.x + jx, (double)L.y + jy);
    }
};

// The summation contract as a running sum: sample s of a pixel, value v, folded into the pixel's state. Samples arrive in ascending s.
// A chunk's first sample and a pixel's first chunk are ASSIGNED, not added to zero, as pt_finish_kernel and the render kernels' chunk loops do (-0.0 stays).
PT_HD void pt_film_fold(PtVec3& total, PtVec3& partial, uint32_t s, PtVec3 v) {
    const uint32_t k = s % PT_SAMPLE_CHUNK;
    partial = k == 0u ? v : partial + v;
    if (k == PT_SAMPLE_CHUNK - 1u) total = s == PT_SAMPLE_CHUNK - 1u ? partial : total + partial;
}
// ... and the sum of a pixel's `count` > 0 samples out of its state: the complete chunks' sum, with the open chunk's behind it.
PT_HD PtVec3 pt_film_sum(PtVec3 total, PtVec3 partial, uint32_t count) {
    if (count % PT_SAMPLE_CHUNK == 0u) return total;
    if (count < PT_SAMPLE_CHUNK) return partial;
    return total + partial;
}

constexpr int pt_film_waves(int /*mode*/) { return 3; }  // the interpreter's three (pt_radiance_waves)

// tex, park: as for the radiance pass
PT_DECLARE_MODE_LAUNCHERS(pt_film_launch_mode_, const PtFilmArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);

// pt_film.hip. Both take the slice / image through PtRenderArgs' fields (width, height, x0 .. y1, n_slots) and queue one kernel on `stream`.
// fold: one thread per pixel slot of the slice; the slot's launch_samples staged samples folded into total / partial in ascending order, count += launch_samples.
hipError_t pt_film_fold_launch(const PtFilmArgs& a, double* total, double* partial, uint32_t* count, hipStream_t stream);
// resolve: one thread per pixel of the image; pixels with count > 0 get rgb (optional) and linear (optional), row-major; the others are not written.
hipError_t pt_film_resolve_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, uint8_t* rgb, double* linear, hipStream_t stream);
