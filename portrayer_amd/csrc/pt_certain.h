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
