// Shadow rays that CERTAINLY end in the tile's cached occluder, settled in f32 before the light's f64 set-up.
//
// A shadow ray only asks whether ANY node is hit in [EPSILON, INF) (material.rs:171-179). Two thirds of big-scene's shadow walks end at the
// probe of the tile's cached occluder (pt_trace_packet), most of them nowhere near that node's silhouette - and each still pays the light's
// direction (f64 sqrt, three f64 divisions) and the exact leaf test. This is the accept-side twin of the walks' conservative f32 culls
// (pt_raypk_axis): a test that can only say "certainly hit"; everything else takes the exact path as before.
//
// THE TABLE (pt_certain_ball, once per node and launch): for spheres and cubes a world-space ball B(c, rho) that lies inside the primitive with room to
// spare, as four floats {c, rho^2}; every other type gets rho^2 = 0 (3.). THE LANE TEST (pt_certain_lane): the f32 line through P~ = f32(P) and L~ = f32(L) has, at a parameter s in [0, 4), a point
// closer than rho to c~ = f32(c).
//
// 1. What the lane test establishes. With v = fl(c~ - P~), w = fl(L~ - P~), ANY s and u = fl(v - s w): the point Q = P + s (L - P) of the exact
//    line has |c - Q| <= |u| + E, where (eps = 2^-24; |c~ - c| <= eps |c|, |P~ - P| <= eps |P|, |L~ - L| <= eps |L|, the two subtractions round
//    by eps |v| and eps |w|, each fma of u by eps |u_k| - relative, it goes into the relative margin; |P| <= |c| + |v|, |L| <= |P| + |w|)
//        E <= eps [ |c| + (|c| + |v|) + |v| + s ( (|c| + |v| + |w|) + (|c| + |v|) + |w| ) ]  =  eps [ (2 + 2 s)(|c| + |v|) + 2 s |w| ].
//    s is NOT required to be the foot of the perpendicular - any point of the ray inside the ball will do - so the quotient's rounding (the host
//    divides, the device multiplies by v_rcp_f32, one ulp off) only moves Q along the line: it enters no bound. What is required: vw > 0 and
//    ww > 0, so s >= 0 (Q lies ahead of the origin or is the origin); s < 4, and s |w| <= |v| (1 + 2^-20) because s^2 ww = s (s ww) and s ww is
//    vw within two roundings, vw <= |v| |w|. So  E <= eps (10 |c| + 12.1 |v|) < 2^-20 |c| + 2^-20 |v|.  |v| <= |u| + s |w| and (s |w|)^2 = s vw
//    (same two roundings; a subnormal s makes s |w| < 1e-18): the test  s vw < 2^24 rho^2  gives s |w| < 2^12 rho, |v| < (2^12 + 1) rho, so the |v| term is below 2^-7.9 rho.
//    Every comparison is written so that a NaN yields "not certain"; an infinity in w makes u NaN; ww that overflows makes s = 0, u = v, and the
//    claim is then about P itself, which is true as it stands; the floor on ww keeps s out of the range where s ww is no longer vw.
//    (The form vv ww - vw^2 is not used: it cancels where the light is far.)
// 2. The table's radius. The reference tests node k in ITS model space through the record inv_k: the "world primitive" is { x : inv(x) in K }, K the
//    unit primitive. For x in B(c, r): |inv(x) - c_m| <= |inv3 (x - c)| + |inv(c) - c_m| <= sqrt(g) r + e, g = the largest Gershgorin row sum of
//    inv3 inv3^T (>= its largest eigenvalue = sigma_max(inv3)^2 - for a rotation times a uniform scale inv3 inv3^T is diagonal and the bound is exact up
//    to rounding), e = the residual of the centre (c = fwd(c_m) is only used as a guess: e is computed, and a record with e > 2^-20 r_m gets no ball).
//    So r = r_m / sqrt(g) keeps B(c, r) inside the primitive up to that 2^-20, and
//        rho = r (1 - 2^-5) - 2^-10 - 2^-20 |c|,   rho^2 rounded down to f32 and once more by 2^-20;   no ball unless rho >= r / 2.
//    Of the 2^-5 r: 2^-7.9 rho pays for the |v| term, 2^-20 for e, 2^-19 for the roundings of u, uu and rho^2; at least 2^-6 r is left. With 1.: the exact
//    line passes, at a parameter t_q >= 0 (world units: the reference's direction is unit length), through a point Q whose ball B(Q, m), m = 2^-10 +
//    2^-6 r, lies inside the primitive. The primitive is convex, so the ray leaves it at t_x >= t_q + m >= 97 EPSILON, through its boundary. Nodes with
//    sigma_max / sigma_min above 2^10 (by the same Gershgorin sums of fwd3 fwd3^T) get no ball: in model space m is still >= 2^-16 of the primitive's size, against
//    f64 rounding of 2^-52 x (|c| + |v|) / r <= 2^-31 in the local ray (|c| <= 2^19 r from rho >= r / 2, |v| <= 2^13 rho).
// 3. The reference's own test then reports a hit (pt_unit_prim_hit over [EPSILON, INF); the origin may lie outside, inside or ON the surface - the
//    common case: the back of the node the primary ray hit). t_x is where the ray leaves the primitive, at least 97 EPSILON ahead:
//    * sphere: the line passes the centre closer than 1 - 2^-16: two roots lo < hi = t_x. lo >= EPSILON: returned; else hi is, being >= 97 EPSILON.
//    * cube: the ray leaves through a face whose own division gives t_x >= EPSILON at a point pt_cube_contains accepts (EPSILON of slack, so edges
//      and corners are no exception). That face is accepted unless an earlier face was (`end` only shrinks after a hit).
//    * cylinder and cone: NO BALL. Their quadrics give up the first root in range only (quirk Q1), and the side test and the cap test are decided by different
//      roundings. Away from the rims and the apex the argument goes through as for the cube (the side where the first root in range lies on the solid, else the
//      cap or base the ray enters or leaves through). But a ray that enters through the RIM circle of a cap to within f64 rounding and leaves through the side may be
//      turned down by both tests (each sees the crossing on the other's side), and a steep ray from inside a cone that passes its APEX closer than about 1e-8 of the cone
//      finds a negative discriminant (it is the square of that distance and drowns in the rounding of its terms): the reference reports nothing where the exact ray
//      passes through the solid. A ball cannot know about either set - every ball inside the solid is met by lines through the rim and through the apex - so a
//      certain answer there would differ from the reference's. tests/test_certain_shadow.py holds such rays (apex offsets from 1e-9) and checks that these types are never certain.
//    plane, triangle, meshes: no interior, no ball.
#pragma once

#include "pt_prims.h"

#define PT_CERTAIN_S_MAX 4.0f
#define PT_CERTAIN_REACH2_LOG2 24  // (s |w|)^2 = s vw < 2^24 rho^2; by v_ldexp_f32 (exact, and an underflow only makes the small smaller): as a factor the constant sat in a register pair from the top of the kernel on
#define PT_CERTAIN_WW_MIN 1e-30f

// The launch's record of one flattened node: out = {c.x, c.y, c.z, rho^2}; rho^2 = 0: never certain.
PT_HD void pt_certain_ball(uint32_t type, const double* fwd, const double* inv, float* out) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    double rm;
    if (type == PT_SPHERE) rm = 1.0;
    else if (type == PT_CUBE) rm = 0.5;
    else return;  // cylinder and cone: the argument does not close (3.); plane, triangle, meshes: no interior
    const PtVec3 cm = pt_v3(0.0, 0.0, 0.0);
    const PtVec3 c = pt_xform_point(fwd, cm);
    const PtVec3 back = pt_xform_point(inv, c) - cm;
    const double e = fabs(back.x) + fabs(back.y) + fabs(back.z);  // >= |inv(c) - c_m|
    double g = 0.0, h = 0.0;  // largest Gershgorin row sums of inv3 inv3^T and fwd3 fwd3^T
    for (int i = 0; i < 3; i++) {
        double gi = 0.0, hi = 0.0;
        for (int j = 0; j < 3; j++) {
            gi += fabs(inv[4 * i] * inv[4 * j] + inv[4 * i + 1] * inv[4 * j + 1] + inv[4 * i + 2] * inv[4 * j + 2]);
            hi += fabs(fwd[4 * i] * fwd[4 * j] + fwd[4 * i + 1] * fwd[4 * j + 1] + fwd[4 * i + 2] * fwd[4 * j + 2]);
        }
        g = gi > g ? gi : g;
        h = hi > h ? hi : h;
    }
    if (!(g > 1e-280 && g < 1e280 && h > 1e-280 && h < 1e280)) return;
    if (!(g * h <= 1048576.0)) return;          // sigma_max / sigma_min <= 2^10
    if (!(e <= 0x1p-20 * rm)) return;           // fwd and inv are no pair
    const double r = (rm / sqrt(g)) * (1.0 - 0x1p-40);
    const double cn = sqrt(pt_dot(c, c));
    const double rho = r * (1.0 - 0x1p-5) - 0x1p-10 - 0x1p-20 * cn;
    if (!(rho >= 0.5 * r)) return;
    const double rho2 = (rho * rho) * (1.0 - 0x1p-20);
    if (!(rho2 > 1e-30 && rho2 < 1e30 && cn < 1e15)) return;
    float f = (float)rho2;
    if ((double)f > rho2) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) - 1u);  // (f is a positive normal number: the next float towards 0)
    out[0] = (float)c.x; out[1] = (float)c.y; out[2] = (float)c.z; out[3] = f;
}

// f32(x) where it is used: the shaded point is the same for every light of an item, and left to itself the compiler converts it once in front of the light loop and
// keeps the three floats (as three register PAIRS, for its packed f32 arithmetic) across the walks - six more spilled registers in the headline instantiation.
PT_HD float pt_f32_here(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    float f;
    asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(f) : "v"(x));
    return f;
#else
    return (float)x;
#endif
}

// One lane: rec = a node's record, (px, py, pz) = f32(P), (lx, ly, lz) = f32(L).
PT_HD bool pt_certain_lane(const float* rec, float px, float py, float pz, float lx, float ly, float lz) {
    const float vx = rec[0] - px, vy = rec[1] - py, vz = rec[2] - pz;
    const float wx = lx - px, wy = ly - py, wz = lz - pz;
    const float ww = __builtin_fmaf(wz, wz, __builtin_fmaf(wy, wy, wx * wx));
    const float vw = __builtin_fmaf(vz, wz, __builtin_fmaf(vy, wy, vx * wx));
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = vw * __builtin_amdgcn_rcpf(ww);
#else
    const float s = vw / ww;
#endif
    const float ux = __builtin_fmaf(-s, wx, vx), uy = __builtin_fmaf(-s, wy, vy), uz = __builtin_fmaf(-s, wz, vz);
    const float uu = __builtin_fmaf(uz, uz, __builtin_fmaf(uy, uy, ux * ux));
    // (& and not &&: five compares and four scalar ands in a straight line, no branch around three fmas)
    return (vw > 0.0f) & (ww > PT_CERTAIN_WW_MIN) & (s < PT_CERTAIN_S_MAX) & (uu < rec[3]) & (__builtin_ldexpf(s * vw, -PT_CERTAIN_REACH2_LOG2) < rec[3]);
}

// DARK LIGHTS: a light enclosed in a solid, settled once per launch.
//
// A shadow ray runs over [EPSILON, INF): nothing bounds it by the light's distance. A point light L that lies inside a closed convex solid is therefore dark everywhere - the
// ray from ANY origin toward L passes through the solid and leaves it. THE TABLE (pt_dark_light, once per light and launch, behind pt_certain_ball's): the lowest node whose
// certain ball encloses L with the margin below, and the bounds of THE LANE GUARD (pt_dark_lane): with P~ = f32(P), L~ = f32(L), w = fl(L~ - P~) and d2 = fl(|w|^2),
//     PT_DARK_D2_MIN <= d2 <= ceil.   Where it holds in every shaded lane, the light is skipped: no occluder entry, no ball record, no direction, no probe, no walk.
//
// 4. The margin. The table's record is {c~, rho~^2}, c~ = f32(c), rho~ <= rho (2.: rho^2 is rounded down twice). pt_dark_light flags L where, in f64,
//        |L - c~|^2 <= rho~^2 (1 - 2^-6)^2 (1 - 2^-40)     (three products, two sums, relative rounding below 2^-50: the 2^-40 pays for them),
//    so |L - c| <= rho (1 - 2^-6) + 2^-24 |c|, and with r - rho = 2^-5 r + 2^-10 + 2^-20 |c| (2.) the ball B(L, m'), m' = 2^-6 rho + 2^-5 r + 2^-10, lies inside B(c, r), which lies
//    inside the primitive up to the 2^-20 r of 2. (e). The reference's ray is {P + t d}, h = fl(L - P), d = fl(h / fl|h|). An f64 difference rounds RELATIVE to its result, so
//    each h_k is (L_k - P_k)(1 + 2^-53) whatever |L| and |P| are; pt_length and the three divisions add relative 2^-51 at most: d is the exact unit direction turned and
//    scaled by less than 2^-50. The exact ray therefore passes, at t_q = (L - P) . d > 0, a point Q with |Q - L| <= 2^-50 |L - P|. The guard's ceiling gives |L - P| < 2^12 rho
//    (5.), so |Q - L| < 2^-38 rho, and B(Q, m), m = 2^-10 + 2^-6 r - the ball 2. ends with - lies inside B(L, m'), with 2^-6 rho and half of the 2^-5 r to spare. The same ceiling
//    gives |c - P| <= |L - P| + |L - c| < (2^12 + 1) rho: 1.'s bound on |v|, which 2. uses for the f64 rounding of the LOCAL ray (|c| <= 2^19 r is the table's). From here 2. and
//    3. apply as they stand: the ray leaves the primitive at t_x >= t_q + m >= 97 EPSILON, and the reference's own test reports a hit.
// 5. The ceiling. |L~ - L| <= eps |L|, |P~ - P| <= eps |P| <= eps (|L| + |L - P|), each w_k rounds by eps |w_k|, d2 by 3 eps relative:
//        |L - P| <= sqrt(d2) (1 + 2^-21) + 2^-22 |L|.   The table stores  ceil = (2^12 rho~ (1 - 2^-10) - 2^-21 |L|)^2  rounded down to f32 (no flag unless the bracket is positive):
//    d2 <= ceil gives |L - P| < 2^12 rho. An overflowing d2 is +inf and fails; a NaN fails both comparisons as they are written.
// 6. The floor. P == L gives the reference h = 0, a NaN direction and so a "lit" verdict: such a lane must take the exact path. d2 >= PT_DARK_D2_MIN = 1e-30 means some
//    |w_k| >= 5.7e-16 (a normal float: no flushed difference decides), so L~_k != P~_k, and as rounding is a function L_k != P_k IN F64, whatever |L| is. One of |L_k|, |P_k| is
//    then at least 2.8e-16, and two distinct doubles the larger of which is M differ by at least 2^-53 M: |h_k| >= 3e-32, its square is a normal double, fl|h| > 0 and d is
//    finite. Nothing else is asked of a short h: 4. holds for every |L - P| > 0 (t_q may be as small as 3e-32; the ray still leaves B(L, m') at least m' ahead of L).
// 7. Every origin. 4. uses nothing about P but the two bounds of the guard. P outside the solid: the ray enters and leaves it. P inside (a second primitive that cuts the solid, a
//    camera inside it looking at its inner surface) or ON its surface (the solid's own shaded points, the common case): the ray passes L and leaves the solid beyond it - 3.'s
//    cases "lo < EPSILON: hi is returned" and "the face the ray leaves through". Points of other nodes are no different: the test is an OR over nodes.
// 8. Types. Cylinder and cone have no ball (3.), so a light inside one is never flagged and takes the exact path. An AREA light (both area vectors non-zero, the kernel's own
//    criterion, light.rs:51-53) is never flagged either: its position is drawn per sample.
#define PT_DARK_D2_MIN 1e-30f
#define PT_DARK_WORDS 8  // per light, in front of the occluder table: {f32(L).xyz, ceil} - what a lane reads; ceil = 0: not dark - then {node + 1, floor, 0, 0} for the tests

// Does the point light of record `light` (15 doubles: position, colour, falloff, area_a, area_b) certainly lie inside the ball `ball` (pt_certain_ball's record)? out[0..3] =
// the lane guard's record {f32(L), ceil}; all zero where it does not.
PT_HD bool pt_dark_light(const double* light, const float* ball, float* out) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    const bool area = !((light[9] == 0.0 && light[10] == 0.0 && light[11] == 0.0) || (light[12] == 0.0 && light[13] == 0.0 && light[14] == 0.0));
    if (area) return false;
    const double rho2 = (double)ball[3];
    if (!(rho2 > 0.0)) return false;
    const PtVec3 l = pt_v3(light[0], light[1], light[2]);
    const PtVec3 d = l - pt_v3((double)ball[0], (double)ball[1], (double)ball[2]);
    if (!(pt_dot(d, d) <= rho2 * ((1.0 - 0x1p-6) * (1.0 - 0x1p-6) * (1.0 - 0x1p-40)))) return false;
    const double reach = sqrt(rho2) * (4096.0 * (1.0 - 0x1p-10)) - 0x1p-21 * sqrt(pt_dot(l, l));
    if (!(reach > 0.0)) return false;
    const double ceil2 = reach * reach;
    if (!(ceil2 > 1e-30 && ceil2 < 1e37)) return false;
    float f = (float)ceil2;
    if ((double)f > ceil2) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) - 1u);  // (a positive normal number: the next float towards 0)
    out[0] = (float)l.x; out[1] = (float)l.y; out[2] = (float)l.z; out[3] = f;
    return true;
}

// One lane: rec = a dark light's record, (px, py, pz) = f32(P). (& and not &&, and the comparisons this way round: a NaN fails)
PT_HD bool pt_dark_lane(const float* rec, float px, float py, float pz) {
    const float wx = rec[0] - px, wy = rec[1] - py, wz = rec[2] - pz;
    const float d2 = __builtin_fmaf(wz, wz, __builtin_fmaf(wy, wy, wx * wx));
    return (d2 >= PT_DARK_D2_MIN) & (d2 <= rec[3]);
}
