// Launchers of the ambient-occlusion pass (pt_ao, include/portrayer_hip.h), one per traversal mode: each is defined in its own object
// (pt_ao_inst.hip compiled with -DPT_INST_MODE=<mode>), like the bounded-segment ray queries' (pt_segments_inst.h), whose walks and rules it shares.
#pragma once

#include "pt_segments_inst.h"
#include "pt_ao.h"

#define PT_AO_POINT_MAJOR 0   // a wavefront = 64 / S consecutive points x S samples
#define PT_AO_SAMPLE_MAJOR 1  // a wavefront = 64 consecutive points, one walk per sample

struct PtAoArgs {
    PtRenderArgs r;            // scene, stack areas, work queues, overflow flag; n_items = wavefronts' worth of work in the layout launched
    uint64_t n;                // points
    const double* positions;   // n x 3
    const double* normals;     // n x 3
    PtAoSet set;               // seed, first_index, pass, flags, bias, eye
    uint32_t samples;          // S: 1, 2, 4, .. 64
    uint32_t log2_samples;
    double radius;             // > PT_EPSILON; +inf: unbounded
    uint32_t* occluded;        // each buffer optional, indexed by point
    uint8_t* valid;
    double* bent;              // n x 3
};

// LDS beside the traversal stacks, per block: every lane's direction, 3 f64, kept there while its walk runs - point-major, the first lane of a point's group sums
// them in sample order afterwards; sample-major, the lane adds it to its sum so far, 3 f64 more.
constexpr size_t pt_ao_frame_bytes(int layout) { return (size_t)PT_BLOCK * 8 * (layout == PT_AO_POINT_MAJOR ? 3 : 6); }

// Waves per SIMD (pt_ao_kernel's launch bounds): the walks are pt_segments_kernel's, so is the choice.
constexpr int pt_ao_waves(int mode) { return pt_segments_waves(mode); }

PT_DECLARE_MODE_LAUNCHERS(pt_ao_launch_mode_, const PtAoArgs& a, int layout, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
