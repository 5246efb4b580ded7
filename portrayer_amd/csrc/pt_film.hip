// The film's two small kernels (pt_film_*, include/portrayer_hip.h) and the host-side replay of its running sum: pt_film_fold_kernel folds what a launch
// of the sampling kernel (pt_film.h) staged into the film's per-pixel state, pt_film_resolve_kernel turns that state into pixels. Both hold the summation
// contract through pt_film_fold / pt_film_sum (pt_film_inst.h) and nothing else; the finishing arithmetic is pt_finish_pixel's (pt_shade.h) with the pixel's
// own count as the divisor.
#include <hip/hip_runtime.h>

#include "../../include/portrayer_hip.h"
#include "pt_film_inst.h"
#include "pt_shade.h"

// One thread per pixel slot of the slice (8x8 tiles over the slice, pt_slot_to_pixel): the slot's staged samples in ascending order.
__global__ void __launch_bounds__(256) pt_film_fold_kernel(PtFilmArgs a, double* __restrict__ total, double* __restrict__ partial, uint32_t* __restrict__ count) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= a.r.n_slots) return;
    uint32_t x, y;
    if (!pt_slot_to_pixel(a.r, slot, &x, &y)) return;
    const size_t p = (size_t)y * a.r.width + x;
    const uint32_t c = count[p];
    double *t = total + 3 * p, *q = partial + 3 * p;
    PtVec3 tot = pt_v3(t[0], t[1], t[2]), par = pt_v3(q[0], q[1], q[2]);
    const double* s = a.staging + 3 * (size_t)slot * a.lw;
    for (uint32_t j = 0; j < a.launch_samples; j++) pt_film_fold(tot, par, c + j, pt_v3(s[3 * j], s[3 * j + 1], s[3 * j + 2]));
    t[0] = tot.x; t[1] = tot.y; t[2] = tot.z;
    q[0] = par.x; q[1] = par.y; q[2] = par.z;
    count[p] = c + a.launch_samples;
}

// One thread per pixel of the image: sum -> mean, gamma, clamp, u8 (pt_finish_pixel with count[p] in place of the render's samples). Pixels without samples
// keep whatever the output buffers hold.
__global__ void __launch_bounds__(256) pt_film_resolve_kernel(uint32_t n_pixels, const double* __restrict__ total, const double* __restrict__ partial,
                                                             const uint32_t* __restrict__ count, uint8_t* __restrict__ rgb, double* __restrict__ linear) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t c = count[p];
    if (c == 0u) return;
    const double *t = total + 3 * (size_t)p, *q = partial + 3 * (size_t)p;
    const PtVec3 sum = pt_film_sum(pt_v3(t[0], t[1], t[2]), pt_v3(q[0], q[1], q[2]), c);
    PtVec3 color = sum / (double)c;
    if (linear) { double* o = linear + 3 * (size_t)p; o[0] = color.x; o[1] = color.y; o[2] = color.z; }
    if (!rgb) return;
    const double g = 1.0 / PT_GAMMA;
    double ch[3] = {pt_pow(color.x, g), pt_pow(color.y, g), pt_pow(color.z, g)};
    uint8_t* o = rgb + 3 * (size_t)p;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double v = ch[k];
        v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        o[k] = pt_to_u8(v);
    }
}

hipError_t pt_film_fold_launch(const PtFilmArgs& a, double* total, double* partial, uint32_t* count, hipStream_t stream) {
    if (a.r.n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_film_fold_kernel, dim3((a.r.n_slots + 255u) / 256u), dim3(256), 0, stream, a, total, partial, count);
    return hipGetLastError();
}

hipError_t pt_film_resolve_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, uint8_t* rgb, double* linear, hipStream_t stream) {
    const uint32_t n = width * height;  // (pt_film_create refuses films of 2^31 pixels or more)
    hipLaunchKernelGGL(pt_film_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, total, partial, count, rgb, linear);
    return hipGetLastError();
}

// Host-side replay (no GPU, no context): n samples given to one pixel in n_cuts consecutive adds of cuts[k] samples each, every add split into launches of
// at most PT_FILM_LW as pt_film_add splits it, every launch folded as pt_film_fold_kernel folds it; out_sum = what pt_film_resolve_kernel divides.
extern "C" int pt_test_film_fold_host(uint32_t n, const double* samples, const uint32_t* cuts, uint32_t n_cuts, double out_sum[3]) {
    if (!samples || !cuts || !out_sum || n == 0 || n_cuts == 0) return PT_ERR_ARGUMENT;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_cuts; k++) sum += cuts[k];
    if (sum != n) return PT_ERR_ARGUMENT;
    PtVec3 tot = pt_v3(0.0, 0.0, 0.0), par = pt_v3(0.0, 0.0, 0.0);
    uint32_t count = 0;
    for (uint32_t k = 0; k < n_cuts; k++)
        for (uint32_t left = cuts[k]; left > 0;) {
            const uint32_t m = left < (uint32_t)PT_FILM_LW ? left : (uint32_t)PT_FILM_LW;
            const uint32_t c = count;
            const double* s = samples + 3 * (size_t)c;
            for (uint32_t j = 0; j < m; j++) pt_film_fold(tot, par, c + j, pt_v3(s[3 * j], s[3 * j + 1], s[3 * j + 2]));
            count = c + m;
            left -= m;
        }
    const PtVec3 r = pt_film_sum(tot, par, count);
    out_sum[0] = r.x; out_sum[1] = r.y; out_sum[2] = r.z;
    return PT_OK;
}
