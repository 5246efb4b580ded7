// Launchers of the render kernel, one per traversal mode: each is defined in its own object
// (pt_render_inst.hip compiled with -DPT_INST_MODE=<mode>) so that the eight sets of kernel
// instantiations compile side by side.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_mode_launch.h"
#include "pt_shade.h"

PT_DECLARE_MODE_LAUNCHERS(pt_launch_mode_, const PtRenderArgs& a, int variant, bool stats, bool tex, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
