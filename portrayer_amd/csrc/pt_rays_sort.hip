// reorder = 1 of the ray-query pass (pt_rays.h): a key per ray, then the library's radix sort over (key, ray index) - the sort the device tree
// build already uses (pt_build.hip). Rays that start near each other and point into the same octant end up in the same wavefront, whose one walk
// then pays for the union of 64 similar paths instead of 64 unrelated ones. The keys decide only WHICH rays share a wavefront; no result depends on that.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "pt_rays_inst.h"

#define PT_RAYS_KEY_BLOCK 256

// 20 bits -> every third bit of 60
__device__ static unsigned long long pt_rays_spread20(uint32_t v) {
    unsigned long long x = v & 0xFFFFFu;
    x = (x | (x << 32)) & 0x000F00000000FFFFull;
    x = (x | (x << 16)) & 0x000F0000FF0000FFull;
    x = (x | (x << 8)) & 0x000F00F00F00F00Full;
    x = (x | (x << 4)) & 0x00C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x0249249249249249ull;
    return x;
}

struct PtRaysKeyBox { double lo[3], scale[3]; };  // cell = (o - lo) * scale, clamped to [0, 2^20 - 1]

__global__ void __launch_bounds__(PT_RAYS_KEY_BLOCK) pt_rays_key_kernel(uint64_t n, const double* __restrict__ origins, const double* __restrict__ directions, PtRaysKeyBox box,
                                                                        unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * PT_RAYS_KEY_BLOCK + threadIdx.x;
    if (i >= n) return;
    PtRay r;
    r.o = pt_v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    r.d = pt_v3(directions[3 * i], directions[3 * i + 1], directions[3 * i + 2]);
    unsigned long long key = 1ull << 63;  // not traced: behind every ray that is
    if (pt_rays_traced(r)) {
        const double o[3] = {r.o.x, r.o.y, r.o.z};
        uint32_t cell[3];
        for (int k = 0; k < 3; k++) {
            double c = (o[k] - box.lo[k]) * box.scale[k];
            c = c < 0.0 ? 0.0 : (c > 1048575.0 ? 1048575.0 : c);  // (finite: |o| <= 1e18, the scale is finite)
            cell[k] = (uint32_t)c;
        }
        const unsigned long long oct = (r.d.x < 0.0 ? 1ull : 0ull) | (r.d.y < 0.0 ? 2ull : 0ull) | (r.d.z < 0.0 ? 4ull : 0ull);
        key = (oct << 60) | pt_rays_spread20(cell[0]) | (pt_rays_spread20(cell[1]) << 1) | (pt_rays_spread20(cell[2]) << 2);
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

hipError_t pt_rays_sort_bytes(uint64_t n, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n, 0u, 64u, (hipStream_t) nullptr);
}

hipError_t pt_rays_sort(uint64_t n, const double* origins, const double* directions, const double lo[3], const double hi[3], unsigned long long* keys_in,
                        unsigned long long* keys_out, uint32_t* vals_in, uint32_t* vals_out, void* tmp, size_t tmp_bytes, hipStream_t stream) {
    PtRaysKeyBox box;
    for (int k = 0; k < 3; k++) {
        const double ext = hi[k] - lo[k];
        const bool usable = ext > 0.0 && ext < 1e300 && fabs(lo[k]) < 1e300;  // (else an empty or unbounded axis: one cell)
        box.lo[k] = usable ? lo[k] : 0.0;
        box.scale[k] = usable ? 1048576.0 / ext : 0.0;
    }
    hipLaunchKernelGGL(pt_rays_key_kernel, dim3((unsigned)((n + PT_RAYS_KEY_BLOCK - 1) / PT_RAYS_KEY_BLOCK)), dim3(PT_RAYS_KEY_BLOCK), 0, stream, n, origins, directions, box, keys_in, vals_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, 64u, stream);
}
