// Launchers of the guides pass, one per traversal mode: each is defined in its own object
// (pt_guides_inst.hip compiled with -DPT_INST_MODE=<mode>), like the primary-visibility pass's (pt_aov_inst.h).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_aov_inst.h"

struct PtGuidesArgs {
    PtRenderArgs r;        // as PtAovArgs::r: one work item per 8x8 tile of the slice
    double off_x, off_y;   // sample position inside the pixel
    double* albedo;        // each buffer optional: full image, row-major
    double* position;
    double* normal;
    int32_t* node;
};

// Compiled for pt_aov_waves(mode) waves per SIMD, the primary-visibility pass's: the two passes share one PtPass, and so one set of stack columns.
// tex: the scene has material maps (PtSceneView::mat_maps) - the TEX = true instantiation; without them the material record alone is read.
PT_DECLARE_MODE_LAUNCHERS(pt_guides_launch_mode_, const PtGuidesArgs& a, bool tex, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
