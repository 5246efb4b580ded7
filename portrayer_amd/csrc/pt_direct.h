// The contract of the direct-light pass (pt_direct, include/portrayer_hip.h): which shadow rays a point casts at the scene's lights and what each
// one that arrives adds. A fixed sequence of correctly rounded f64 operations (+, -, *, /, sqrt, fmax; no fused multiply-add: the build passes -ffp-contract=off)
// over the point, its normal and the light's 15 doubles, as PT_HD functions - the kernel (pt_direct_inst.hip) and the host replay (pt_test_direct_host, pt_api.hip)
// compile this very text, and tests/test_direct_contract.py compares a numpy restatement (tests/direct_restate.py) with it in every bit.
//
// Point i of a call has the stream index q = first_index + i, S = samples. In this order:
//   1. valid      all six components of P and N finite and at most 1e18 in magnitude (pt_rays' rule), and N != (0, 0, 0): pt_ao's step 1. An invalid point casts nothing.
//   2. face eye   PT_AO_FACE_EYE: v = P - eye; if dot(N, v) > 0 then N = -N.                                                         (pt_ao's step 2)
//   3. normalise  nrm = N / sqrt(dot(N, N)), component-wise.                                                                          (pt_ao's step 3)
//   4. origin     o = P + nrm bias.
//   5. light      light li = {position, colour, falloff c0 c1 c2, area a, area b}. A POINT light iff a == (0, 0, 0) or b == (0, 0, 0) (light.rs:51-53): lpos =
//                 position for every k. Else lpos = position + (a ca + b cb), ca = 2 rng(seed, q S + k, pass, 2 j) - 1, cb = 2 rng(seed, q S + k, pass, 2 j + 1) - 1,
//                 j = the number of area lights with an index below li; q S + k is a 64-bit product and sum, reduced modulo 2^64 only.
//   6. shadow ray v = lpos - o; dist = sqrt(dot(v, v)); d = v / dist; t_max = +inf, with PT_DIRECT_TO_LIGHT t_max = dist.
//   7. cosine     c = fmax(dot(nrm, d), 0). c == 0 or c NaN: the sample contributes nothing and casts no ray.
//   8. occlusion  the ray (o, d) is a ray of pt_segments with that t_max and any_hit = 1: traced under pt_segments_traced's rule (a ray it would not trace
//                 contributes nothing), occluded iff that pass says so.
//   9. term       att = (c0 + c1 dist) + (c2 dist) dist (light.rs:31-33); term = (colour c) / att per channel.
//  10. sum        from (0, 0, 0) and lit = 0, li ascending and inside it k = 0 .. S - 1 ascending: a sample that contributes and is not occluded adds its term, left to
//                 right, and 1 to lit. A point light's sample is the same for every k: it is traced once and added S times.
#pragma once

#include "pt_math.h"

#define PT_DIRECT_FLAG_FACE_EYE 1u  // == PT_AO_FACE_EYE (include/portrayer_hip.h)
#define PT_DIRECT_FLAG_TO_LIGHT 2u  // == PT_DIRECT_TO_LIGHT

// What a call fixes for all of its points.
struct PtDirectSet {
    uint64_t seed, first_index;
    uint32_t pass, flags;
    uint32_t samples;
    double bias;
    PtVec3 eye;
};

// Step 1 (pt_ao_valid's rule, restated).
PT_HD bool pt_direct_valid(PtVec3 P, PtVec3 N) {
    const double lim = 1e18;
    const bool in_range = fabs(P.x) <= lim && fabs(P.y) <= lim && fabs(P.z) <= lim && fabs(N.x) <= lim && fabs(N.y) <= lim && fabs(N.z) <= lim;  // (false for NaN and inf)
    return in_range && !(N.x == 0.0 && N.y == 0.0 && N.z == 0.0);
}

// Steps 2 to 4. The caller has checked pt_direct_valid.
PT_HD void pt_direct_point(const PtDirectSet& s, PtVec3 P, PtVec3 N, PtVec3* o, PtVec3* nrm) {
    if (s.flags & PT_DIRECT_FLAG_FACE_EYE) {
        const PtVec3 v = P - s.eye;
        if (pt_dot(N, v) > 0.0) N = -N;
    }
    *nrm = N / sqrt(pt_dot(N, N));
    *o = P + *nrm * s.bias;
}

// Step 5's test: does light[15] sample nothing?
PT_HD bool pt_direct_is_point_light(const double* light) {
    return (light[9] == 0.0 && light[10] == 0.0 && light[11] == 0.0) || (light[12] == 0.0 && light[13] == 0.0 && light[14] == 0.0);  // light.rs:51-53
}

// Step 5 for sample k of the point with stream index q; j = the area lights in front of this one.
PT_HD PtVec3 pt_direct_light_position(const PtDirectSet& s, const double* light, uint32_t j, uint64_t q, uint32_t k) {
    const PtVec3 pos = pt_v3(light[0], light[1], light[2]);
    if (pt_direct_is_point_light(light)) return pos;
    const uint64_t stream = q * (uint64_t)s.samples + k;  // modulo 2^64
    const double ca = 2.0 * pt_rng_f64(s.seed, stream, s.pass, 2u * j) - 1.0;
    const double cb = 2.0 * pt_rng_f64(s.seed, stream, s.pass, 2u * j + 1u) - 1.0;
    return pos + (pt_v3(light[9], light[10], light[11]) * ca + pt_v3(light[12], light[13], light[14]) * cb);
}

// Steps 6, 7 and 9, and step 8's rule for which rays are traced (pt_segments_traced, restated): does the sample cast a ray? If so *d, *t_max and *term are that
// ray's; if not they are zeros.
PT_HD bool pt_direct_sample(const PtDirectSet& s, PtVec3 o, PtVec3 nrm, PtVec3 lpos, const double* light, PtVec3* d, double* t_max, PtVec3* term) {
    const PtVec3 v = lpos - o;
    const double dist = sqrt(pt_dot(v, v));
    const PtVec3 dir = v / dist;
    const double tm = (s.flags & PT_DIRECT_FLAG_TO_LIGHT) ? dist : (double)INFINITY;
    const double c = fmax(pt_dot(nrm, dir), 0.0);
    const double lim = 1e18;
    const bool in_range = fabs(o.x) <= lim && fabs(o.y) <= lim && fabs(o.z) <= lim && fabs(dir.x) <= lim && fabs(dir.y) <= lim && fabs(dir.z) <= lim;  // (false for NaN and inf)
    const bool casts = c > 0.0 && in_range && tm > PT_EPSILON;  // (c > 0: the direction is not all zero; false for a NaN c)
    *d = pt_v3(0.0, 0.0, 0.0); *t_max = 0.0; *term = pt_v3(0.0, 0.0, 0.0);
    if (!casts) return false;
    const double att = (light[6] + light[7] * dist) + (light[8] * dist) * dist;
    *d = dir; *t_max = tm;
    *term = (pt_v3(light[3], light[4], light[5]) * c) / att;
    return true;
}
