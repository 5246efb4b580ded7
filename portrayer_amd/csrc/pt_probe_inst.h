// The probe pass (pt_probe, include/portrayer_hip.h): the argument block of its kernel, the source policy that makes the interpreter
// (pt_source_advance, pt_radiance.h) shade the probe contract's rays (pt_probe.h), and the launchers - one per traversal mode, each in its own object
// (pt_probe_inst.hip compiled with -DPT_INST_MODE=<mode>), like the gather pass's - and the launcher of the fold over a probe's rounds (pt_probe.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "pt_radiance_inst.h"
#include "pt_probe.h"

struct PtProbeArgs {
    PtRenderArgs r;            // scene, seed, recursion frames, stack areas, work queues, overflow flag; n_items = n x R wavefronts, item w = (probe w / R, round w % R).
                               // FIRST: the kernel re-reads the block through the kernarg segment (pt_args_again), and pt_kd_layout & co. take a PtRenderArgs
    uint64_t n;                // probes of this launch
    const double* positions;   // n x 3
    PtProbeSet set;            // seed, first_index (the stream index of this launch's probe 0), pass: what pt_probe_dir reads (set.seed == r.seed)
    uint32_t samples;          // S: 64, 128, 256, 512 or 1024
    uint32_t log2_rounds;      // R = S / 64 = 1 << log2_rounds
    double background[3];      // the call's colour: what a ray that leaves the scene brings back
    double* sh;                // R == 1: n x 27, the kernel's own store; R > 1: null here (the fold writes it)
    double* partial;           // R > 1: n x R x 27, item w's 27 sums at partial + 27 w; R == 1: null. Both null: only `valid` is wanted and nothing is traced
    uint8_t* valid;            // n, optional
};
static_assert(offsetof(PtProbeArgs, r) == 0, "the kernel reads PtRenderArgs at the start of its argument block");

// The probe pass's source (SRC of pt_source_advance / pt_source_light_position), PtGatherSource's twin. The lane carries its probe's index IN THE LAUNCH in L.x
// (< n <= PT_PROBE_MAX = 2^20) and its sample k (< 1024) in L.y, two fields the interpreter and the walks never read or write, and its ray - the probe's position
// and pt_probe_dir's direction - in L.ray from the moment its sample starts. The generator's stream is that of ray (q, k) of pt_radiance over the flattened
// rays: q * S + k with q = first_index + probe, a 64-bit product of 64-bit factors reduced modulo 2^64 only - the same value as pt_radiance's stream_base + i
// with stream_base = first_index * S, i = probe * S + k.
struct PtProbeSource {
    uint64_t first_index, samples;
    uint32_t pass;
    PtVec3 bg;
    PT_HD uint32_t sample(const PtRenderArgs&, const PtLane&) const { return pass; }
    PT_HD uint64_t stream(const PtRenderArgs&, const PtLane& L) const { return (first_index + (uint64_t)L.x) * samples + (uint64_t)L.y; }
    PT_HD PtVec3 background(const PtRenderArgs&, const PtLane&) const { return bg; }
    PT_HD PtRay primary(const PtRenderArgs&, const PtLane& L) const { return L.ray; }
};

constexpr int pt_probe_waves(int /*mode*/) { return 3; }  // the interpreter's three (pt_radiance_waves)

// tex, park: as for the radiance pass
PT_DECLARE_MODE_LAUNCHERS(pt_probe_launch_mode_, const PtProbeArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);

// pt_probe.hip: sh[p][t] = partial[p][0][t] + partial[p][1][t] + ... in ascending round, left to right; one thread per (probe, value)
hipError_t pt_probe_fold_launch(const double* partial, double* sh, uint64_t n, uint32_t rounds, hipStream_t stream);
