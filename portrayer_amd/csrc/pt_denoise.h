// The film's denoiser (pt_film_denoise*, include/portrayer_hip.h): an edge-avoiding a-trous wavelet filter over the film's resolved mean, steered
// by the primary-visibility buffers (pt_aov: position, normal, node) and by the film's own noise estimate (pt_film_error_of). It has no counterpart in the
// reference, so it is DEFINED here, as a fixed sequence of correctly rounded IEEE f64 operations - + - * /, comparisons, no exp, no libm: the kernels
// (pt_denoise.hip, both forms), the host replay (pt_test_denoise_host) and a numpy restatement (tests/test_denoise_host.py) agree in every bit because all of
// them are these functions, in this order. The weights are compact rationals (1 - x)^2 clamped at 0, not exp(-x), for exactly that reason.
//
// Per level the filter reads a (c, v) pair per pixel - colour and the variance of the colour's channel sum - and writes the next level's: two work buffers of
// 32 bytes per pixel (c.x, c.y, c.z, v), which BELONG TO THE FILM: allocated by its first denoise, reused by every later one, freed with the film.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/portrayer_hip.h"
#include "pt_math.h"

#define PT_DENOISE_EPS 1e-12
#define PT_DENOISE_MAX_ITERATIONS 8
#define PT_DENOISE_MAX_NORMAL_POWER_LOG2 7

// The call's constants, derived once on the host in f64.
struct PtDenoiseConst {
    double kc;            // sigma_color * sigma_color
    double kp;            // 1.0 / (sigma_plane * sigma_plane)
    int32_t normal_pow;   // normal_power_log2: squarings of the clamped dot; < 0 = no normal weight
    uint32_t same_node;   // PT_DENOISE_SAME_NODE
    uint32_t use_color;   // sigma_color > 0
    uint32_t use_plane;   // sigma_plane > 0
};
PT_HD PtDenoiseConst pt_denoise_const(const pt_denoise_params& p) {
    PtDenoiseConst k;
    k.kc = p.sigma_color * p.sigma_color;
    k.kp = p.sigma_plane > 0.0 ? 1.0 / (p.sigma_plane * p.sigma_plane) : 0.0;
    k.normal_pow = p.normal_power_log2;
    k.same_node = (p.flags & PT_DENOISE_SAME_NODE) ? 1u : 0u;
    k.use_color = p.sigma_color > 0.0 ? 1u : 0u;
    k.use_plane = p.sigma_plane > 0.0 ? 1u : 0u;
    return k;
}

// What the filter knows of one pixel at one level. n and pos are read only where the constants ask for them.
struct PtDenoisePix {
    PtVec3 c;
    double v;
    PtVec3 n, pos;
    int32_t node;
};

// Level 0's variance of a pixel with count > 0: the square of pt_film_error_of where the film knows one, the sample's own magnitude at count 1 (nothing is
// known: there is no infinity in the pipeline), 0 on a film without moments (accepted with sigma_color == 0 only). `c` is resolve's linear, `err` the error.
PT_HD double pt_denoise_seed_variance(PtVec3 c, uint32_t count, bool moments, double err) {
    if (!moments) return 0.0;
    if (count >= 2u) return err * err;
    const double my = (c.x + c.y) + c.z;
    return my * my;
}

// H = {1/16, 1/4, 3/8, 1/4, 1/16} at k = -2 .. 2; every product of two of them is exact.
PT_HD double pt_denoise_h(int k) { return k == 0 ? 0.375 : ((k == 1 || k == -1) ? 0.25 : 0.0625); }

// The weight of tap (i, j) of centre p at q, both with count > 0 and inside the film: steps 1 to 5 of the contract. 0 = skipped.
PT_HD double pt_denoise_weight(const PtDenoiseConst& k, int i, int j, const PtDenoisePix& p, const PtDenoisePix& q) {
    const bool miss_p = p.node < 0, miss_q = q.node < 0;
    if (miss_p != miss_q) return 0.0;
    if (k.same_node && p.node != q.node) return 0.0;
    double w = pt_denoise_h(j) * pt_denoise_h(i);
    if (!miss_p && k.normal_pow >= 0) {
        double a = (p.n.x * q.n.x + p.n.y * q.n.y) + p.n.z * q.n.z;
        a = a > 0.0 ? a : 0.0;
        for (int s = 0; s < k.normal_pow; s++) a = a * a;
        w = w * a;
    }
    if (!miss_p && k.use_plane) {
        const double ex = q.pos.x - p.pos.x, ey = q.pos.y - p.pos.y, ez = q.pos.z - p.pos.z;
        const double d = (p.n.x * ex + p.n.y * ey) + p.n.z * ez;
        const double t = 1.0 - (d * d) * k.kp;
        w = w * (t > 0.0 ? t * t : 0.0);
    }
    if (k.use_color) {
        const double yp = (p.c.x + p.c.y) + p.c.z, yq = (q.c.x + q.c.y) + q.c.z;
        const double dy = yp - yq;
        const double t = 1.0 - (dy * dy) / (k.kc * (p.v + q.v) + PT_DENOISE_EPS);
        w = w * (t > 0.0 ? t * t : 0.0);
    }
    return w;
}

// The running sums of a centre: started at +0, taps added in the order j = -2 .. 2 outer, i = -2 .. 2 inner.
struct PtDenoiseAcc {
    PtVec3 cs;
    double vs, ws;
};
PT_HD PtDenoiseAcc pt_denoise_acc_zero() {
    PtDenoiseAcc a;
    a.cs = pt_v3(0.0, 0.0, 0.0);
    a.vs = 0.0;
    a.ws = 0.0;
    return a;
}
// Steps 6 and 7: a weight that is not > 0 (0, negative, NaN from non-finite guides) adds nothing.
PT_HD void pt_denoise_accumulate(PtDenoiseAcc& a, PtVec3 cq, double vq, double w) {
    if (!(w > 0.0)) return;
    a.cs.x = a.cs.x + cq.x * w;
    a.cs.y = a.cs.y + cq.y * w;
    a.cs.z = a.cs.z + cq.z * w;
    a.vs = a.vs + (w * w) * vq;
    a.ws = a.ws + w;
}
// The level's output at the centre; ws == 0 (a degenerate guide at the centre itself) passes the input through.
PT_HD void pt_denoise_level_out(const PtDenoiseAcc& a, PtVec3 cp, double vp, PtVec3* c, double* v) {
    if (a.ws == 0.0) { *c = cp; *v = vp; return; }
    c->x = a.cs.x / a.ws;
    c->y = a.cs.y / a.ws;
    c->z = a.cs.z / a.ws;
    *v = a.vs / (a.ws * a.ws);
}

// Albedo demodulation (pt_film_denoise_albedo*): level 0's colour is divided by the diffuse colour under the pixel before the levels smooth it and
// multiplied by it again after the last one, so that texture detail the guides know of is not blurred. The levels themselves are the ones above, unchanged.
#define PT_DENOISE_ALBEDO_EPS 0.0078125  // 2^-7, exact: a black albedo divides by this

// The modulation of one channel of a hit pixel's albedo guide: a NaN, negative or infinite channel is not demodulated (and makes no NaN).
PT_HD double pt_denoise_modulation_of(double a) { return (a >= 0.0 && a < INFINITY) ? a + PT_DENOISE_ALBEDO_EPS : 1.0; }
// The modulation of a pixel with count > 0: its albedo's where the node guide says hit, (1, 1, 1) on a miss.
PT_HD PtVec3 pt_denoise_modulation(int32_t node, PtVec3 albedo) {
    if (node < 0) return pt_v3(1.0, 1.0, 1.0);
    return pt_v3(pt_denoise_modulation_of(albedo.x), pt_denoise_modulation_of(albedo.y), pt_denoise_modulation_of(albedo.z));
}
// The film keeps ONE variance, that of the channel sum: it is scaled by the square of the mean modulation - exact for grey albedos, an approximation otherwise.
PT_HD double pt_denoise_mean_modulation(PtVec3 m) { return ((m.x + m.y) + m.z) / 3.0; }
// After the level-0 seed ...
PT_HD void pt_denoise_demodulate(PtVec3 m, PtVec3* c, double* v) {
    const double mm = pt_denoise_mean_modulation(m);
    c->x = c->x / m.x;
    c->y = c->y / m.y;
    c->z = c->z / m.z;
    *v = *v / (mm * mm);
}
// ... and after the last level, with the pixel's own m.
PT_HD void pt_denoise_remodulate(PtVec3 m, PtVec3* c, double* v) {
    const double mm = pt_denoise_mean_modulation(m);
    c->x = c->x * m.x;
    c->y = c->y * m.y;
    c->z = c->z * m.z;
    *v = *v * (mm * mm);
}

// The tiled form's geometry (pt_denoise.hip): a block owns PT_DN_TILE x PT_DN_TILE pixels of one residue class modulo the step and stages a
// (PT_DN_TILE + 4)^2 neighbourhood of it, every component as an f64 array of its own.
#define PT_DN_TILE 16
#define PT_DN_HALO 2
#define PT_DN_SIDE (PT_DN_TILE + 2 * PT_DN_HALO)
#define PT_DN_CELLS (PT_DN_SIDE * PT_DN_SIDE)
#define PT_DN_LDS_BYTES (PT_DN_CELLS * (10 * 8 + 4 + 4))  // c, v, n, pos as f64; node and valid as words

// One level's launch: in / out are the film's work buffers (4 f64 per pixel), the guides the caller's (normal / position may be null where unused).
struct PtDenoiseLevelArgs {
    PtDenoiseConst k;
    uint32_t width, height;
    uint32_t step;
    const double* in;
    double* out;
    const uint32_t* count;
    const double* position;
    const double* normal;
    const int32_t* node;
};

// pt_denoise.hip. What every entry point refuses of the parameters and the guides (no HIP call): nullptr = fine, else the reason.
const char* pt_denoise_check(const pt_denoise_params* p, const pt_denoise_guides* g);
// Each of the following queues one kernel on `stream`.
// seed: level 0's (c, v) of every pixel with count > 0 out of the film's state (q null: a film without moments).
hipError_t pt_denoise_seed_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, double* work, hipStream_t stream);
// one level, direct (tiled = false: a thread per pixel, 25 taps from global memory) or tiled (LDS-staged residue classes); the same bits either way.
hipError_t pt_denoise_level_launch(const PtDenoiseLevelArgs& a, bool tiled, hipStream_t stream);
// finish: the last level's (c, v) to the caller's buffers, each optional; rgb is resolve's finishing of c. Pixels with count == 0 are not written.
hipError_t pt_denoise_finish_launch(uint32_t width, uint32_t height, const double* work, const uint32_t* count, uint8_t* rgb, double* linear, double* variance, hipStream_t stream);
// pt_denoise_albedo.hip: the seed with the division by the modulation fused in, the finish with the products; node and albedo are the caller's guides.
hipError_t pt_denoise_albedo_seed_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, const int32_t* node,
                                         const double* albedo, double* work, hipStream_t stream);
hipError_t pt_denoise_albedo_finish_launch(uint32_t width, uint32_t height, const double* work, const uint32_t* count, const int32_t* node, const double* albedo, uint8_t* rgb, double* linear,
                                           double* variance, hipStream_t stream);
