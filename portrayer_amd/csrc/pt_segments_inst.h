// Launchers of the bounded-segment ray queries (pt_segments, include/portrayer_hip.h), one per traversal mode: each is defined in its own object
// (pt_segments_inst.hip compiled with -DPT_INST_MODE=<mode>), like the ray-query pass's (pt_rays_inst.h), whose arguments, rules and sort it shares.
#pragma once

#include "pt_rays_inst.h"

struct PtSegmentsArgs {
    PtRaysArgs q;          // everything pt_rays_kernel takes, meaning the same
    const double* t_max;   // n: the exclusive end of ray i's range [PT_EPSILON, t_max[i]), in units of its direction like t
};

// Which rays are traced: pt_rays' rule, and a range that is not empty. (false for a NaN bound)
PT_HD bool pt_segments_traced(const PtRay& r, double t_max) { return pt_rays_traced(r) && t_max > PT_EPSILON; }

// Waves per SIMD (pt_segments_kernel's launch bounds): the walks and the surface code are pt_rays_kernel's, so is the choice.
constexpr int pt_segments_waves(int mode) { return pt_rays_waves(mode); }

PT_DECLARE_MODE_LAUNCHERS(pt_segments_launch_mode_, const PtSegmentsArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
