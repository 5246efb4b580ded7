// Launchers of the ray-query pass (pt_rays, include/portrayer_hip.h), one per traversal mode: each is defined in its own object
// (pt_rays_inst.hip compiled with -DPT_INST_MODE=<mode>), like the primary-visibility pass's (pt_aov_inst.h). Also what the pass's
// two other device steps share with the cast kernel: which rays are traced at all (pt_rays_traced) and the keying + sort of reorder = 1
// (pt_rays_sort.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_mode_launch.h"
#include "pt_shade.h"

struct PtRaysArgs {
    PtRenderArgs r;             // scene, stack areas, work queues, overflow flag; n_items = wavefronts' worth of rays (64 each)
    uint64_t n;                 // rays
    const double* origins;      // n x 3
    const double* directions;   // n x 3
    const uint32_t* perm;       // reorder = 1: slot -> ray index (sorted by key); null: slot == ray index
    int32_t any;                // 1: occlusion query
    double* t;                  // each buffer optional, n entries, indexed by RAY
    double* position;
    double* normal;
    int32_t* node;
    int32_t* sub;
    int32_t* material;
    uint8_t* occluded;
};

// Which rays are traced. Every component finite, the direction not all zero, and every component at most 1e18 in magnitude: that is the bound
// pt_scene_upload guarantees for box coordinates and the one under which every product of the f32 slab constants (pt_raypk_axis, pt_ray32_axis:
// |1 / d| <= 1e18 or the axis is switched off; origin x reciprocal <= 1e36) stays finite, and a reciprocal of at least 1e-18 keeps the constants'
// relative margins meaningful (a product that falls below the normal range is covered by their absolute terms). A direction component BELOW 1e-18
// needs no rule: its axis is switched off, which accepts every box.
PT_HD bool pt_rays_traced(const PtRay& r) {
    const double lim = 1e18;
    const bool in_range = fabs(r.o.x) <= lim && fabs(r.o.y) <= lim && fabs(r.o.z) <= lim && fabs(r.d.x) <= lim && fabs(r.d.y) <= lim && fabs(r.d.z) <= lim;  // (false for NaN and inf)
    return in_range && !(r.d.x == 0.0 && r.d.y == 0.0 && r.d.z == 0.0);
}

// Waves per SIMD the instantiation of a mode is compiled for (pt_rays_kernel's launch bounds), chosen as pt_aov_waves chooses: the modes that carry
// the per-lane KDMesh walker need its registers.
constexpr int pt_rays_waves(int mode) { return (mode == PT_MODE_KD || mode == PT_MODE_FLAT_KDMESH || mode == PT_MODE_HIER) ? 3 : 4; }

PT_DECLARE_MODE_LAUNCHERS(pt_rays_launch_mode_, const PtRaysArgs& a, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);

// reorder = 1 (pt_rays_sort.hip). Key of a ray, most significant first: bit 63 set = not traced (sorts last); bits 62..60 the direction's sign bits
// (z, y, x: set where the component is below zero); bits 59..0 the Morton code of the origin, 20 bits per axis, quantised inside
// the box [lo, hi] (clamped to it). pt_rays_sort_bytes: the sort's temporary storage for n pairs. pt_rays_sort: keys_in / vals_in (the keys and
// 0 .. n - 1) are written by the keying kernel, the stable radix sort leaves the permutation in vals_out.
hipError_t pt_rays_sort_bytes(uint64_t n, size_t* bytes);
hipError_t pt_rays_sort(uint64_t n, const double* origins, const double* directions, const double lo[3], const double hi[3], unsigned long long* keys_in,
                        unsigned long long* keys_out, uint32_t* vals_in, uint32_t* vals_out, void* tmp, size_t tmp_bytes, hipStream_t stream);
