// The demodulated denoise's own kernels (pt_film_denoise_albedo*, include/portrayer_hip.h) and its host replay. The levels are pt_denoise.o's,
// unchanged; what is new sits at the two ends, fused into the kernels that are there anyway, so no extra pass goes over the work buffers:
//   SEED    pt_denoise_seed_kernel's level 0 (pt_film_sum, pt_film_error_of, pt_denoise_seed_variance), then pt_denoise_demodulate by the pixel's modulation;
//   FINISH  pt_denoise_remodulate by the same modulation, then pt_denoise_finish_pixel.
// One thread per pixel, 256-thread blocks, no LDS.
#include <hip/hip_runtime.h>

#include "../../include/portrayer_hip.h"
#include "pt_denoise.h"
#include "pt_denoise_pixel.h"

__global__ void __launch_bounds__(256) pt_albedo_seed_kernel(uint32_t n_pixels, const double* __restrict__ total, const double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                            const double* __restrict__ q2, const int32_t* __restrict__ node, const double* __restrict__ albedo, double* __restrict__ work) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const uint32_t n = count[p];
    if (n == 0u) return;
    const double *t = total + 3 * (size_t)p, *q = partial + 3 * (size_t)p;
    const PtVec3 tot = pt_v3(t[0], t[1], t[2]), par = pt_v3(q[0], q[1], q[2]);
    PtVec3 c = pt_film_sum(tot, par, n) / (double)n;  // pt_denoise_seed_kernel's level 0: resolve's `linear` ...
    const double err = q2 && n >= 2u ? pt_film_error_of(tot, par, q2[p], n) : 0.0;
    double v = pt_denoise_seed_variance(c, n, q2 != nullptr, err);  // ... and its variance
    const double* al = albedo + 3 * (size_t)p;
    pt_denoise_demodulate(pt_denoise_modulation(node[p], pt_v3(al[0], al[1], al[2])), &c, &v);
    double* o = work + 4 * (size_t)p;
    o[0] = c.x; o[1] = c.y; o[2] = c.z;
    o[3] = v;
}

__global__ void __launch_bounds__(256) pt_albedo_finish_kernel(uint32_t n_pixels, const double* __restrict__ work, const uint32_t* __restrict__ count, const int32_t* __restrict__ node,
                                                              const double* __restrict__ albedo, uint8_t* __restrict__ rgb, double* __restrict__ linear, double* __restrict__ variance) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    if (count[p] == 0u) return;
    const double *cv = work + 4 * (size_t)p, *al = albedo + 3 * (size_t)p;
    PtVec3 c = pt_v3(cv[0], cv[1], cv[2]);
    double v = cv[3];
    pt_denoise_remodulate(pt_denoise_modulation(node[p], pt_v3(al[0], al[1], al[2])), &c, &v);
    pt_denoise_finish_pixel(p, c, &v, rgb, linear, variance);
}

hipError_t pt_denoise_albedo_seed_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, const int32_t* node,
                                         const double* albedo, double* work, hipStream_t stream) {
    const uint32_t n = width * height;  // (pt_film_create refuses films of 2^31 pixels or more)
    hipLaunchKernelGGL(pt_albedo_seed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, total, partial, count, q, node, albedo, work);
    return hipGetLastError();
}

hipError_t pt_denoise_albedo_finish_launch(uint32_t width, uint32_t height, const double* work, const uint32_t* count, const int32_t* node, const double* albedo, uint8_t* rgb, double* linear,
                                           double* variance, hipStream_t stream) {
    const uint32_t n = width * height;
    hipLaunchKernelGGL(pt_albedo_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, work, count, node, albedo, rgb, linear, variance);
    return hipGetLastError();
}

// Host-side replay (no GPU, no context): pt_test_denoise_host's levels between the two steps of pt_denoise.h, from a level-0 input the caller supplies.
extern "C" int pt_test_denoise_albedo_host(uint32_t width, uint32_t height, const pt_denoise_params* params, const double* linear, const double* variance, const uint32_t* counts,
                                           const pt_denoise_guides* guides, const double* albedo, double* out_linear, double* out_variance) {
    if (pt_denoise_check(params, guides) || !albedo || !linear || !counts || (!out_linear && !out_variance) || width == 0 || height == 0 || (uint64_t)width * height >= 0x80000000ull)
        return PT_ERR_ARGUMENT;
    if (!variance && params->sigma_color > 0.0) return PT_ERR_ARGUMENT;
    const size_t n = (size_t)width * height;
    double *c0 = new double[3 * n], *v0 = new double[n], *c1 = new double[3 * n], *v1 = new double[n];
    auto modulation = [&](size_t p) { return pt_denoise_modulation(guides->node[p], pt_v3(albedo[3 * p], albedo[3 * p + 1], albedo[3 * p + 2])); };
    for (size_t p = 0; p < n; p++) {
        PtVec3 c = pt_v3(linear[3 * p], linear[3 * p + 1], linear[3 * p + 2]);
        double v = variance ? variance[p] : 0.0;
        if (counts[p] != 0u) pt_denoise_demodulate(modulation(p), &c, &v);  // (a pixel without samples is neither centre nor tap)
        c0[3 * p] = c.x; c0[3 * p + 1] = c.y; c0[3 * p + 2] = c.z;
        v0[p] = v;
        c1[3 * p] = c1[3 * p + 1] = c1[3 * p + 2] = v1[p] = 0.0;
    }
    const int rc = pt_test_denoise_host(width, height, params, c0, v0, counts, guides, c1, v1);
    if (rc == PT_OK)
        for (size_t p = 0; p < n; p++) {
            if (counts[p] == 0u) continue;  // left untouched, as in resolve
            PtVec3 c = pt_v3(c1[3 * p], c1[3 * p + 1], c1[3 * p + 2]);
            double v = v1[p];
            pt_denoise_remodulate(modulation(p), &c, &v);
            if (out_linear) { out_linear[3 * p] = c.x; out_linear[3 * p + 1] = c.y; out_linear[3 * p + 2] = c.z; }
            if (out_variance) out_variance[p] = v;
        }
    delete[] c0;
    delete[] v0;
    delete[] c1;
    delete[] v1;
    return rc;
}
