// The contract of the probe pass (pt_probe, include/portrayer_hip.h): which rays a probe - a point in free space, no normal - casts over the
// whole sphere, and the nine order-2 spherical-harmonic basis values each ray's radiance is weighted with. A fixed sequence of correctly rounded f64 operations
// (+, -, *, /, sqrt; no fused multiply-add: the build passes -ffp-contract=off) over the position and the tables of constants (pt_probe_tables.h and pt_ao's
// PT_AO_ROT), as PT_HD functions - the kernel (pt_probe_inst.hip) and the host replay (pt_test_probe_host, pt_api.hip) compile this very text, and
// tests/probe_restate.py restates it in numpy and tests/test_probe_contract.py compares every bit.
//
// Probe i of a call has the stream index q = first_index + i. In this order:
//   1. valid      the three components of P finite and at most 1e18 in magnitude (pt_rays' rule). An invalid probe casts nothing.
//   2. rotation   j = (uint32)(pt_rng_f64(seed, q, pass, 0) * 256.0); (c, s) = PT_AO_ROT[j].
//                 m = (uint32)(pt_rng_f64(seed, q, pass, 1) * 1024.0); the axis N = PT_PROBE_DIRS[m].
//   3. direction  sample k, (x, y, z) = PT_PROBE_DIRS[k], then pt_ao.h's steps 3, 5, 6 and 7 with that N, restated here (pt_ao.h stays as it is):
//                 n = N / sqrt(dot(N, N)); lx = c x - s y, ly = s x + c y, lz = z;
//                 sg = copysign(1, n.z); a = -1 / (sg + n.z); b = (n.x n.y) a;
//                 T = (1 + ((sg n.x) n.x) a, sg b, -(sg n.x)); B = (b, sg + (n.y n.y) a, -n.y);        (branch-free, every product left to right)
//                 d = (T lx + B ly) + n lz per component, NOT renormalised. The origin is P itself: no bias, no face-eye step.
//   4. radiance   what pt_radiance answers for (P, d_k) with the stream (seed, q * S + k, sample = pass): the kernel's business (PtProbeSource).
//   5. basis      c0 .. c4 = PT_PROBE_SH, every product left to right:
//                 Y0 = c0, Y1 = c1 d.y, Y2 = c1 d.z, Y3 = c1 d.x, Y4 = (c2 d.x) d.y, Y5 = (c2 d.y) d.z, Y6 = c3 ((3 d.z) d.z - 1), Y7 = (c2 d.x) d.z,
//                 Y8 = c4 (d.x d.x - d.y d.y).
//   6. sum        per round r of 64 samples and per (coefficient i, channel c): from 0, + Y_i(d_k) rgb_k[c] for k = 64 r .. 64 r + 63 ascending; sh[i][c] is
//                 round 0's partial plus the later rounds' in ascending r (pt_probe_inst.hip, pt_probe.hip).
#pragma once

#include "pt_math.h"
#include "pt_ao_tables.h"
#include "pt_probe_tables.h"

#define PT_PROBE_VALUES 27u  // 9 coefficients x 3 channels: value t = 3 i + c

// What a call fixes for all of its probes.
struct PtProbeSet {
    uint64_t seed, first_index;
    uint32_t pass;
};

// Step 1.
PT_HD bool pt_probe_valid(PtVec3 P) {
    const double lim = 1e18;
    return fabs(P.x) <= lim && fabs(P.y) <= lim && fabs(P.z) <= lim;  // (false for NaN and inf)
}

// Steps 2 and 3 for sample k (< 1024) of the probe with stream index q: its ray's direction.
PT_HD PtVec3 pt_probe_dir(const PtProbeSet& s, uint64_t q, uint32_t k) {
    const uint32_t j = (uint32_t)(pt_rng_f64(s.seed, q, s.pass, 0) * 256.0);   // < 256: the draw is below 1
    const uint32_t m = (uint32_t)(pt_rng_f64(s.seed, q, s.pass, 1) * 1024.0);  // < 1024
    const double c = PT_AO_ROT[j][0], sn = PT_AO_ROT[j][1];
    const PtVec3 N = pt_v3(PT_PROBE_DIRS[m][0], PT_PROBE_DIRS[m][1], PT_PROBE_DIRS[m][2]);
    const PtVec3 n = N / sqrt(pt_dot(N, N));
    const double x = PT_PROBE_DIRS[k][0], y = PT_PROBE_DIRS[k][1], z = PT_PROBE_DIRS[k][2];
    const double lx = c * x - sn * y;
    const double ly = sn * x + c * y;
    const double sg = copysign(1.0, n.z);
    const double a = -1.0 / (sg + n.z);
    const double b = (n.x * n.y) * a;
    const PtVec3 T = pt_v3(1.0 + ((sg * n.x) * n.x) * a, sg * b, -(sg * n.x));
    const PtVec3 B = pt_v3(b, sg + (n.y * n.y) * a, -n.y);
    return (T * lx + B * ly) + n * z;
}

// Step 5.
PT_HD void pt_probe_basis(PtVec3 d, double Y[9]) {
    const double c0 = PT_PROBE_SH[0], c1 = PT_PROBE_SH[1], c2 = PT_PROBE_SH[2], c3 = PT_PROBE_SH[3], c4 = PT_PROBE_SH[4];
    Y[0] = c0;
    Y[1] = c1 * d.y;
    Y[2] = c1 * d.z;
    Y[3] = c1 * d.x;
    Y[4] = (c2 * d.x) * d.y;
    Y[5] = (c2 * d.y) * d.z;
    Y[6] = c3 * ((3.0 * d.z) * d.z - 1.0);
    Y[7] = (c2 * d.x) * d.z;
    Y[8] = c4 * (d.x * d.x - d.y * d.y);
}
