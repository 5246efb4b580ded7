// Launchers of the primary-visibility pass, one per traversal mode: each is defined in its own object
// (pt_aov_inst.hip compiled with -DPT_INST_MODE=<mode>), like the render kernels' (pt_render_inst.h).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_mode_launch.h"
#include "pt_shade.h"

struct PtAovArgs {
    PtRenderArgs r;        // scene, camera, slice and tile geometry as for a render of one sample per pixel (n_items = tiles), stack areas, work counter, overflow flag
    double off_x, off_y;   // sample position inside the pixel
    double* depth;         // each buffer optional: full image, row-major
    double* position;
    double* normal;
    int32_t* node;
    int32_t* sub;
    int32_t* material;
};

// Waves per SIMD the instantiation of a mode is compiled for (pt_aov_kernel's launch bounds) - and so how much LDS a block may take for its stacks (pt_walk_sizing):
// the modes that carry the per-lane KDMesh walker need its registers, as in a render.
constexpr int pt_aov_waves(int mode) { return (mode == PT_MODE_KD || mode == PT_MODE_FLAT_KDMESH || mode == PT_MODE_HIER) ? 3 : 4; }

PT_DECLARE_MODE_LAUNCHERS(pt_aov_launch_mode_, const PtAovArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
