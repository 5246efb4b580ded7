// Launchers of the radiance pass (pt_radiance, include/portrayer_hip.h), one per traversal mode: each is defined in its own object
// (pt_radiance_inst.hip compiled with -DPT_INST_MODE=<mode>), like the ray-query pass's (pt_rays_inst.h). Also the pass's argument block and
// its source policy: where the interpreter (pt_source_advance, pt_radiance.h) gets a lane's primary ray, background colour and generator stream from.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_rays_inst.h"

struct PtRadianceArgs {
    PtRenderArgs r;             // scene, seed, recursion frames, stack areas, work queues, overflow flag; n_items = wavefronts' worth of rays (64 each).
                                // FIRST: the kernel re-reads the block through the kernarg segment (pt_args_again), and pt_kd_layout & co. take a PtRenderArgs
    uint64_t n;                 // rays
    const double* origins;      // n x 3
    const double* directions;   // n x 3
    const uint32_t* perm;       // reorder = 1: slot -> ray index (pt_rays_sort.hip); null: slot == ray index
    const double* background;   // 3 doubles, or n x 3 indexed by RAY
    uint32_t bg_stride;         // 0: one colour for every ray; 3: a colour per ray
    uint32_t sample;            // third word of the generator's counter
    uint64_t stream_base;       // ray i draws from stream (r.seed, stream_base + i, sample)
    double* rgb;                // n x 3, indexed by RAY
};
static_assert(offsetof(PtRadianceArgs, r) == 0, "the kernel reads PtRenderArgs at the start of its argument block");

// The radiance pass's source (SRC of pt_source_advance / pt_source_light_position): the lane carries its ray's INDEX in L.x and the ray itself in L.ray when its
// sample starts (pt_radiance_kernel loads it to decide whether it is traced at all). The stream belongs to the index, not to the lane or the slot the ray
// runs in: which rays share a wavefront, and in which order they are taken, changes no draw.
struct PtRaySource {
    const double* bg;
    uint32_t bg_stride, sample_index;
    uint64_t stream_base;
    PT_HD uint32_t sample(const PtRenderArgs&, const PtLane&) const { return sample_index; }
    PT_HD uint64_t stream(const PtRenderArgs&, const PtLane& L) const { return stream_base + L.x; }
    PT_HD PtVec3 background(const PtRenderArgs&, const PtLane& L) const {
        const double* b = bg + (size_t)bg_stride * L.x;
        return pt_v3(b[0], b[1], b[2]);
    }
    PT_HD PtRay primary(const PtRenderArgs&, const PtLane& L) const { return L.ray; }
};

// Waves per SIMD every instantiation is compiled for: the interpreter's three (PT_INTERP_WAVES, pt_render_kernel.h) - its state machine wants the 168 registers
// whatever the traversal mode.
constexpr int pt_radiance_waves(int /*mode*/) { return 3; }

// tex: the scene has texture or normal maps (TEX instantiation); park: its hits spawn rays (PARK = 1: the youngest parked recursion frame stays in LDS)
PT_DECLARE_MODE_LAUNCHERS(pt_radiance_launch_mode_, const PtRadianceArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
