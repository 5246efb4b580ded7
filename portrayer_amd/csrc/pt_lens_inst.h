// The film's lens (pt_film_add_lens, include/portrayer_hip.h): the argument block of its sampling kernel, the source policy that makes the
// interpreter (pt_source_advance, pt_radiance.h) take the lens contract's primary rays (pt_lens.h), and the launchers - one per traversal mode, each in its
// own object (pt_lens_inst.hip compiled with -DPT_INST_MODE=<mode>). Everything else of a lens add is the film's: PtFilmArgs, the staging buffer, the fold.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_film_inst.h"
#include "pt_lens.h"

struct PtLensArgs {
    PtFilmArgs f;    // what pt_film_kernel takes, unchanged. FIRST: the kernel re-reads the block through the kernarg segment (pt_args_again), and the
                     // interpreter and the walks take the PtRenderArgs at its start
    PtLensSet lens;  // model, aperture, focus, extent: the same in every lane
};
static_assert(offsetof(PtLensArgs, f) == 0, "the kernel reads PtFilmArgs (and PtRenderArgs) at the start of its argument block");

// The lens film's source (SRC of pt_source_advance / pt_source_light_position): PtFilmSource except for the primary ray. `lens` points into the argument block
// as the kernarg segment shows it (pt_args_again): the four fields are scalar loads where a sample starts, not registers carried across the walks.
struct PtLensSource {
    const PtLensSet* lens;
    PT_HD uint32_t sample(const PtRenderArgs&, const PtLane& L) const { return L.item; }
    PT_HD uint64_t stream(const PtRenderArgs& a, const PtLane& L) const { return (uint64_t)L.y * a.width + L.x; }
    PT_HD PtVec3 background(const PtRenderArgs& a, const PtLane& L) const { return pt_background(a, L.x, L.y); }
    PT_HD PtRay primary(const PtRenderArgs& a, const PtLane& L) const {  // pt_lane_advance's PT_ST_NEW_SAMPLE
        const uint64_t pixel = (uint64_t)L.y * a.width + L.x;
        double jx, jy;
        pt_lens_jitter(a.seed, a.jitter_mode == PT_JITTER_RNG, pixel, L.item, &jx, &jy);
        return pt_lens_ray(a.cam, *lens, a.seed, pixel, L.item, (double)L.x + jx, (double)L.y + jy);
    }
};

constexpr int pt_lens_waves(int /*mode*/) { return 3; }  // the interpreter's three (pt_radiance_waves)

// tex, park: as for the radiance pass
PT_DECLARE_MODE_LAUNCHERS(pt_lens_launch_mode_, const PtLensArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
