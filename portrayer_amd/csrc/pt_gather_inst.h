// The gather pass (pt_gather, include/portrayer_hip.h): the argument block of its kernel, the source policy that makes the interpreter
// (pt_source_advance, pt_radiance.h) shade the ambient-occlusion contract's rays (pt_ao.h), and the launchers - one per traversal mode, each in its own
// object (pt_gather_inst.hip compiled with -DPT_INST_MODE=<mode>), like the radiance pass's and the film's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_radiance_inst.h"
#include "pt_ao.h"

struct PtGatherArgs {
    PtRenderArgs r;            // scene, seed, recursion frames, stack areas, work queues, overflow flag; n_items = wavefronts' worth of points (64 / S each).
                               // FIRST: the kernel re-reads the block through the kernarg segment (pt_args_again), and pt_kd_layout & co. take a PtRenderArgs
    uint64_t n;                // points
    const double* positions;   // n x 3
    const double* normals;     // n x 3
    PtAoSet set;               // seed, first_index, pass, flags, bias, eye: what pt_ao_ray reads (set.seed == r.seed)
    uint32_t samples;          // S: 1, 2, 4, .. 64
    uint32_t log2_samples;
    double background[3];      // the call's colour: what a ray that leaves the scene brings back
    double* sum;               // n x 3; each buffer optional, indexed by point
    uint8_t* valid;
};
static_assert(offsetof(PtGatherArgs, r) == 0, "the kernel reads PtRenderArgs at the start of its argument block");

// The gather pass's source (SRC of pt_source_advance / pt_source_light_position). The lane carries its point's index IN THE CALL in L.x (< n <= PT_AO_MAX = 2^24)
// and its sample k in L.y, two fields the interpreter and the walks never read or write, and its ray - steps 1 to 8 of pt_ao's contract - in L.ray from the
// moment its sample starts (pt_gather_kernel makes it there, because whether the lane is traced at all is a question about that ray). The generator's stream is
// that of ray (q, k) of pt_radiance over the flattened rays: q * S + k with q = first_index + point, a 64-bit product of 64-bit factors - no 32-bit field of
// the lane ever holds q or the product - and the same value modulo 2^64 as pt_radiance's stream_base + i with stream_base = first_index * S, i = point * S + k.
struct PtGatherSource {
    uint64_t first_index, samples;
    uint32_t pass;
    PtVec3 bg;
    PT_HD uint32_t sample(const PtRenderArgs&, const PtLane&) const { return pass; }
    PT_HD uint64_t stream(const PtRenderArgs&, const PtLane& L) const { return (first_index + (uint64_t)L.x) * samples + (uint64_t)L.y; }
    PT_HD PtVec3 background(const PtRenderArgs&, const PtLane&) const { return bg; }
    PT_HD PtRay primary(const PtRenderArgs&, const PtLane& L) const { return L.ray; }
};

// Steps 1 to 8 for lane (point p, sample k) of a call: false, and a zero ray, for an invalid point.
PT_HD bool pt_gather_ray(const PtGatherArgs& g, uint64_t p, uint32_t k, PtRay* ray) {
    const double* P = g.positions + 3 * (size_t)p;
    const double* N = g.normals + 3 * (size_t)p;
    const PtVec3 Pv = pt_v3(P[0], P[1], P[2]), Nv = pt_v3(N[0], N[1], N[2]);
    ray->o = ray->d = pt_v3(0.0, 0.0, 0.0);
    if (!pt_ao_valid(Pv, Nv)) return false;
    pt_ao_ray(g.set, Pv, Nv, g.set.first_index + p, k, &ray->o, &ray->d);
    return true;
}

constexpr int pt_gather_waves(int /*mode*/) { return 3; }  // the interpreter's three (pt_radiance_waves)

// tex, park: as for the radiance pass
PT_DECLARE_MODE_LAUNCHERS(pt_gather_launch_mode_, const PtGatherArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);
