// Launchers of the direct-light pass (pt_direct, include/portrayer_hip.h), one per traversal mode: each is defined in its own object
// (pt_direct_inst.hip compiled with -DPT_INST_MODE=<mode>), like the ambient-occlusion pass's (pt_ao_inst.h), whose walks and rules it shares.
#pragma once

#include "pt_segments_inst.h"
#include "pt_direct.h"

struct PtDirectArgs {
    PtRenderArgs r;            // scene (its lights among it), stack areas, work queues, overflow flag; n_items = wavefronts of 64 consecutive points
    uint64_t n;                // points
    const double* positions;   // n x 3
    const double* normals;     // n x 3
    PtDirectSet set;           // seed, first_index, pass, flags, samples, bias, eye
    double* sum;               // each buffer optional, indexed by point; n x 3
    uint32_t* lit;
    uint8_t* valid;
};

// LDS beside the traversal stacks, per block: every lane's term, 3 f64, kept there while its walk runs, and its sum so far, 3 f64 more - pt_ao_kernel's
// sample-major frame.
constexpr size_t pt_direct_frame_bytes() { return (size_t)PT_BLOCK * 8 * 6; }

// Waves per SIMD (pt_direct_kernel's launch bounds): the walks are pt_segments_kernel's, so is the choice.
constexpr int pt_direct_waves(int mode) { return pt_segments_waves(mode); }

PT_DECLARE_MODE_LAUNCHERS(pt_direct_launch_mode_, const PtDirectArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
