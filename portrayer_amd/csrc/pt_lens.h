// The contract of the film's lens (pt_film_add_lens, include/portrayer_hip.h): which primary ray sample s of pixel (x, y) casts through a thin
// lens, an orthographic or a stereographic (fisheye) camera. A fixed sequence of correctly rounded f64 operations (+, -, *, /, sqrt; no fused multiply-add:
// the build passes -ffp-contract=off) over the camera, the lens and pt_ao's two tables of constants (pt_ao_tables.h), as PT_HD functions - the kernel
// (pt_lens_inst.hip) and the host replay (pt_test_lens_rays_host, pt_api.hip) compile this very text, and tests/lens_restate.py restates it in numpy and
// tests/test_lens_contract.py compares every bit.
//
// Sample s of pixel (x, y) of a film `width` pixels wide, pixel = y width + x; the camera's own width and height (pt_camera: what pt_camera_ray divides by)
// are cw and ch. In this order, every product left to right:
//   1. jitter     PT_SAMPLE_RNG: jx, jy = draws 0 and 1 of (seed, pixel, s); PT_SAMPLE_CENTRE: (0.5, 0.5). sx = x + jx, sy = y + jy (PtFilmSource::primary's).
//                 ndc_x = sx / cw, ndc_y = sy / ch.
//   2. THIN       view_y = (1 - 2 ndc_y) fov_factor, view_x = ((2 ndc_x - 1) aspect) fov_factor, world = view_to_world (view_x, view_y, -1): pt_camera_ray's
//                 expressions. D = world - eye. aperture == 0: the ray is pt_camera_ray(cam, sx, sy) itself, (eye, D / |D|), and steps 3 and 4 are skipped.
//   3. lens point k = s & 63, r = s >> 6; j = (uint32)(pt_rng_f64(seed, pixel, 0x80000000 | r, 0) * 256.0); (c, sn) = PT_AO_ROT[j]; (px, py) = the first two
//                 components of PT_AO_DIRS[k]; lx = c px - sn py, ly = sn px + c py. (The xy of the cosine-weighted table is a stratified uniform unit disc,
//                 every power-of-two prefix of it too; a pixel's count cannot pass 2^31, so the sample index 0x80000000 | r is no real sample's.)
//   4. ray        R, U = columns 0 and 1 of view_to_world's upper 3x3, read as entries; e = (R lx + U ly) aperture per component; o = eye + e;
//                 d = pt_normalized(D - e / focus).
//   5. ORTHO      vx = ((2 ndc_x - 1) aspect) extent, vy = (1 - 2 ndc_y) extent; o = view_to_world (vx, vy, 0);
//                 d = pt_normalized(view_to_world (vx, vy, -1) - o).
//   6. STEREO     u = ((2 ndc_x - 1) aspect) extent, v = (1 - 2 ndc_y) extent; q = u u + v v; world = view_to_world (2 u, 2 v, q - 1); o = eye;
//                 d = pt_normalized(world - eye).
// The ray (o, d) is then a ray of pt_radiance with stream pixel, sample s and the pixel's background.
#pragma once

#include "pt_shade.h"
#include "pt_ao_tables.h"

#define PT_LENS_MODEL_THIN 0    // == PT_LENS_THIN (include/portrayer_hip.h)
#define PT_LENS_MODEL_ORTHO 1   // == PT_LENS_ORTHO
#define PT_LENS_MODEL_STEREO 2  // == PT_LENS_STEREO

// What a call fixes for all of its samples: pt_lens' fields (the kernel's argument block carries them in this form).
struct PtLensSet {
    int32_t model;
    double aperture, focus, extent;
};

// Step 1's draws for sample s of the pixel with stream index `pixel`. rng: PT_SAMPLE_RNG (== PT_JITTER_RNG).
PT_HD void pt_lens_jitter(uint64_t seed, bool rng, uint64_t pixel, uint32_t s, double* jx, double* jy) {
    *jx = 0.5; *jy = 0.5;
    if (rng) {  // render.rs:38-39: x drawn before y
        *jx = pt_rng_f64(seed, pixel, s, 0);
        *jy = pt_rng_f64(seed, pixel, s, 1);
    }
}

// Step 3: sample s's point on the unit disc.
PT_HD void pt_lens_point(uint64_t seed, uint64_t pixel, uint32_t s, double* lx, double* ly) {
    const uint32_t k = s & 63u, r = s >> 6;
    const uint32_t j = (uint32_t)(pt_rng_f64(seed, pixel, 0x80000000u | r, 0) * 256.0);  // < 256: the draw is below 1
    const double c = PT_AO_ROT[j][0], sn = PT_AO_ROT[j][1];
    const double px = PT_AO_DIRS[k][0], py = PT_AO_DIRS[k][1];
    *lx = c * px - sn * py;
    *ly = sn * px + c * py;
}

// Steps 2 to 6 for sample s of the pixel with stream index `pixel`, at the jittered position (sx, sy). The caller has checked the lens (pt_lens_error, pt_api.hip).
PT_HD PtRay pt_lens_ray(const PtCamera& c, const PtLensSet& l, uint64_t seed, uint64_t pixel, uint32_t s, double sx, double sy) {
    PtRay r;
    if (l.model == PT_LENS_MODEL_THIN) {
        if (l.aperture == 0.0) return pt_camera_ray(c, sx, sy);
        const double ndc_y = sy / c.height;
        const double view_y = (1.0 - 2.0 * ndc_y) * c.fov_factor;
        const double ndc_x = sx / c.width;
        const double view_x = (2.0 * ndc_x - 1.0) * c.aspect * c.fov_factor;
        const PtVec3 eye = pt_v3(c.eye[0], c.eye[1], c.eye[2]);
        const PtVec3 world = pt_xform_point(c.view_to_world, pt_v3(view_x, view_y, -1.0));
        const PtVec3 D = world - eye;
        double lx, ly;
        pt_lens_point(seed, pixel, s, &lx, &ly);
        const PtVec3 R = pt_v3(c.view_to_world[0], c.view_to_world[4], c.view_to_world[8]);
        const PtVec3 U = pt_v3(c.view_to_world[1], c.view_to_world[5], c.view_to_world[9]);
        const PtVec3 e = (R * lx + U * ly) * l.aperture;
        r.o = eye + e;
        r.d = pt_normalized(D - e / l.focus);
        return r;
    }
    const double ndc_y = sy / c.height;
    const double ndc_x = sx / c.width;
    const double u = (2.0 * ndc_x - 1.0) * c.aspect * l.extent;
    const double v = (1.0 - 2.0 * ndc_y) * l.extent;
    if (l.model == PT_LENS_MODEL_ORTHO) {
        r.o = pt_xform_point(c.view_to_world, pt_v3(u, v, 0.0));
        r.d = pt_normalized(pt_xform_point(c.view_to_world, pt_v3(u, v, -1.0)) - r.o);
        return r;
    }
    const double q = u * u + v * v;
    const PtVec3 eye = pt_v3(c.eye[0], c.eye[1], c.eye[2]);
    const PtVec3 world = pt_xform_point(c.view_to_world, pt_v3(2.0 * u, 2.0 * v, q - 1.0));
    r.o = eye;
    r.d = pt_normalized(world - eye);
    return r;
}
