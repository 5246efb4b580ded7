// The per-pixel body of the denoiser's finish kernels, shared by pt_denoise.hip and pt_denoise_albedo.hip: a (c, v) to the caller's
// buffers. Device code of the two objects that include it. (The seed kernels share pt_film_sum, pt_film_error_of and pt_denoise_seed_variance; pt_denoise.hip's
// is left as it was, so that pt_denoise.o keeps its code object.)
#pragma once

#include "pt_denoise.h"
#include "pt_film_map_inst.h"
#include "pt_shade.h"

// The last level's record of pixel p (colour, and *v read only where the variance is wanted) to the caller's buffers, each optional; rgb by resolve's finishing (pt_film_resolve_kernel).
static __device__ __forceinline__ void pt_denoise_finish_pixel(uint32_t p, PtVec3 color, const double* v, uint8_t* __restrict__ rgb, double* __restrict__ linear, double* __restrict__ variance) {
    if (linear) { double* o = linear + 3 * (size_t)p; o[0] = color.x; o[1] = color.y; o[2] = color.z; }
    if (variance) variance[p] = *v;
    if (!rgb) return;
    const double g = 1.0 / PT_GAMMA;
    double ch[3] = {pt_pow(color.x, g), pt_pow(color.y, g), pt_pow(color.z, g)};
    uint8_t* o = rgb + 3 * (size_t)p;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double v1 = ch[k];
        v1 = v1 < 0.0 ? 0.0 : (v1 > 1.0 ? 1.0 : v1);
        o[k] = pt_to_u8(v1);
    }
}
