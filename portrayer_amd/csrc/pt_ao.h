// The contract of the ambient-occlusion pass (pt_ao, include/portrayer_hip.h): which rays a point casts. A fixed sequence of correctly rounded
// f64 operations (+, -, *, /, sqrt; no fused multiply-add: the build passes -ffp-contract=off) over the point, its normal and two tables of constants
// (pt_ao_tables.h), as PT_HD functions - the kernel (pt_ao_inst.hip) and the host replay (pt_test_ao_rays_host, pt_api.hip) compile this very text, and
// tests/test_ao_contract.py restates it in numpy and compares every bit.
//
// Point i of a call has the stream index q = first_index + i. In this order:
//   1. valid      all six components of P and N finite and at most 1e18 in magnitude (pt_rays' rule), and N != (0, 0, 0). An invalid point casts nothing.
//   2. face eye   PT_AO_FACE_EYE: v = P - eye; if dot(N, v) > 0 then N = -N.
//   3. normalise  n = N / sqrt(dot(N, N)), component-wise. (pt_aov's normals are normalised, a caller's need not be.)
//   4. rotation   j = (uint32)(pt_rng_f64(seed, q, pass, 0) * 256.0); (c, s) = PT_AO_ROT[j].
//   5. local      sample k, (x, y, z) = PT_AO_DIRS[k]: lx = c x - s y, ly = s x + c y, lz = z.
//   6. frame      sg = copysign(1, n.z); a = -1 / (sg + n.z); b = (n.x n.y) a;
//                 T = (1 + ((sg n.x) n.x) a, sg b, -(sg n.x)); B = (b, sg + (n.y n.y) a, -n.y).     (branch-free, every product left to right)
//   7. direction  d = (T lx + B ly) + n lz per component, NOT renormalised (|d| is within 5e-16 of 1).
//   8. origin     o = P + n bias.
// The ray (o, d) is then a ray of pt_segments with t_max = radius and any_hit = 1: traced under pt_segments_traced's rule, occluded iff that pass says so.
#pragma once

#include "pt_math.h"
#include "pt_ao_tables.h"

#define PT_AO_FLAG_FACE_EYE 1u  // == PT_AO_FACE_EYE (include/portrayer_hip.h)

// What a call fixes for all of its points.
struct PtAoSet {
    uint64_t seed, first_index;
    uint32_t pass, flags;
    double bias;
    PtVec3 eye;
};

// Step 1.
PT_HD bool pt_ao_valid(PtVec3 P, PtVec3 N) {
    const double lim = 1e18;
    const bool in_range = fabs(P.x) <= lim && fabs(P.y) <= lim && fabs(P.z) <= lim && fabs(N.x) <= lim && fabs(N.y) <= lim && fabs(N.z) <= lim;  // (false for NaN and inf)
    return in_range && !(N.x == 0.0 && N.y == 0.0 && N.z == 0.0);
}

// Steps 2 to 8 for sample k of the point with stream index q. The caller has checked pt_ao_valid.
PT_HD void pt_ao_ray(const PtAoSet& s, PtVec3 P, PtVec3 N, uint64_t q, uint32_t k, PtVec3* o, PtVec3* d) {
    if (s.flags & PT_AO_FLAG_FACE_EYE) {
        const PtVec3 v = P - s.eye;
        if (pt_dot(N, v) > 0.0) N = -N;
    }
    const PtVec3 n = N / sqrt(pt_dot(N, N));
    const uint32_t j = (uint32_t)(pt_rng_f64(s.seed, q, s.pass, 0) * 256.0);  // < 256: the draw is below 1
    const double c = PT_AO_ROT[j][0], sn = PT_AO_ROT[j][1];
    const double x = PT_AO_DIRS[k][0], y = PT_AO_DIRS[k][1], z = PT_AO_DIRS[k][2];
    const double lx = c * x - sn * y;
    const double ly = sn * x + c * y;
    const double sg = copysign(1.0, n.z);
    const double a = -1.0 / (sg + n.z);
    const double b = (n.x * n.y) * a;
    const PtVec3 T = pt_v3(1.0 + ((sg * n.x) * n.x) * a, sg * b, -(sg * n.x));
    const PtVec3 B = pt_v3(b, sg + (n.y * n.y) * a, -n.y);
    *d = (T * lx + B * ly) + n * z;
    *o = P + n * s.bias;
}
