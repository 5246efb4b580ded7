// The probe pass's small kernel (pt_probe, include/portrayer_hip.h): with S = 64 R samples per probe and R > 1, pt_probe_kernel
// (pt_probe_inst.hip) leaves one partial of 27 sums per (probe, round); pt_probe_fold_kernel adds a probe's rounds. Step 6 of the contract (pt_probe.h): round
// 0's partial plus the later rounds' in ascending round, left to right.
#include <hip/hip_runtime.h>

#include "pt_probe_inst.h"

// One thread per (probe, value): value t of probe p's round r is partial[(p R + r) 27 + t].
__global__ void __launch_bounds__(256) pt_probe_fold_kernel(const double* __restrict__ partial, double* __restrict__ sh, uint64_t values, uint32_t rounds) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= values) return;
    const uint64_t p = idx / PT_PROBE_VALUES, t = idx - p * PT_PROBE_VALUES;
    const double* src = partial + p * rounds * PT_PROBE_VALUES + t;
    double acc = src[0];
    for (uint32_t r = 1; r < rounds; r++) acc = acc + src[(size_t)r * PT_PROBE_VALUES];
    sh[idx] = acc;
}

hipError_t pt_probe_fold_launch(const double* partial, double* sh, uint64_t n, uint32_t rounds, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t values = n * PT_PROBE_VALUES;  // (n <= PT_PROBE_MAX = 2^20)
    hipLaunchKernelGGL(pt_probe_fold_kernel, dim3((uint32_t)((values + 255u) / 256u)), dim3(256), 0, stream, partial, sh, values, rounds);
    return hipGetLastError();
}
