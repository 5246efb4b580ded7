// The chart pass's three kernels (pt_chart, include/portrayer_hip.h; the contract: pt_chart.h) and the host-side replay of the contract.
//   seed     the owner map filled with PT_CHART_NONE
//   own      every triangle rasterised over its box of texels (pt_chart_box), atomicMin(&owner[q], t) where it covers: the lowest index wins whatever the schedule
//   resolve  one thread per texel: the owner's weights again, its records, the node's matrices through the scalar cache, the outputs
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/portrayer_hip.h"
#include "pt_chart.h"
#include "pt_shade.h"

// A box is cut into tiles of at most PT_CHART_TILE x PT_CHART_TILE texels; a triangle's tiles are dealt to the wavefronts (t, blockIdx.y) round robin, so a
// triangle that covers a whole 4096 x 4096 map is the work of gridDim.y wavefronts, not of one. gridDim.y is what brings the launch to about PT_CHART_WAVES
// wavefronts - PT_CHART_WAVES / n_tris, at least 1 (a mesh of a million triangles has none to spare for a second dimension: its empty wavefronts would be the
// launch's cost) and at most the tiles of the whole map (a wavefront beyond its triangle's tile count has nothing to do) and the grid's limit.
#define PT_CHART_TILE 32
#define PT_CHART_WAVES 65536u

__global__ void __launch_bounds__(256) pt_chart_seed_kernel(uint32_t n, uint32_t* __restrict__ owner) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) owner[q] = PT_CHART_NONE;
}

// One wavefront per (triangle, blockIdx.y); the lanes stride a tile's texels.
__global__ void __launch_bounds__(256) pt_chart_own_kernel(PtChartArgs a) {
    const uint32_t t = PT_UNIFORM_U32(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (t >= a.n_tris) return;
    double uv[6], st[6], o;
#pragma unroll
    for (int k = 0; k < 6; k++) uv[k] = a.uv[6 * (size_t)t + k];
    if (!pt_chart_corners(uv, a.width, a.height, st)) return;
    if (!pt_chart_orientation(st, &o)) return;
    int32_t x0, y0, x1, y1;
    if (!pt_chart_box(st, a.width, a.height, &x0, &y0, &x1, &y1)) return;
    // (0 <= x0 <= x1 < width, 0 <= y0 <= y1 < height from here on: every q below is inside the owner map)
    const uint32_t tiles_x = ((uint32_t)(x1 - x0) + PT_CHART_TILE) / PT_CHART_TILE, tiles_y = ((uint32_t)(y1 - y0) + PT_CHART_TILE) / PT_CHART_TILE;
    const uint32_t n_tiles = tiles_x * tiles_y;
    for (uint32_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
        const uint32_t bx = (uint32_t)x0 + tx * PT_CHART_TILE, by = (uint32_t)y0 + ty * PT_CHART_TILE;
        const uint32_t w = min((uint32_t)PT_CHART_TILE, (uint32_t)x1 - bx + 1u), h = min((uint32_t)PT_CHART_TILE, (uint32_t)y1 - by + 1u);
        for (uint32_t k = lane; k < w * h; k += 64u) {
            const uint32_t x = bx + k % w, y = by + k / w;
            double wt[4];
            if (pt_chart_covers(st, o, (double)x + 0.5, (double)y + 0.5, wt)) atomicMin(&a.owner[(size_t)y * a.width + x], t);
        }
    }
}

// One thread per texel. The node's matrices are the same 21 doubles for every lane of the launch: two round trips through the scalar cache per wavefront.
__global__ void __launch_bounds__(256) pt_chart_resolve_kernel(PtChartArgs a) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = a.width * a.height;
    double fwd[12], nrm[9];
    pt_sload_mat12(a.fwd, fwd);
    pt_sload_mat9(a.nrm, nrm);
    if (q >= n) return;
    const uint32_t t = a.owner[q];
    PtVec3 P = pt_v3(0.0, 0.0, 0.0), N = pt_v3(0.0, 0.0, 0.0);
    const bool owned = t != PT_CHART_NONE;  // (then t < n_tris: the own kernel wrote nothing else)
    if (owned && (a.position || a.normal)) {
        double uv[6], st[6], o, wt[4];
#pragma unroll
        for (int k = 0; k < 6; k++) uv[k] = a.uv[6 * (size_t)t + k];
        pt_chart_corners(uv, a.width, a.height, st);
        pt_chart_orientation(st, &o);
        pt_chart_covers(st, o, (double)(q % a.width) + 0.5, (double)(q / a.width) + 0.5, wt);
        PtVec3 p, nm;
        pt_chart_surface(a.tri_v + 9 * (size_t)t, a.tri_n ? a.tri_n + 9 * (size_t)t : nullptr, wt, &p, &nm);
        pt_chart_world(fwd, nrm, a.flags, p, nm, &P, &N);
    }
    if (a.position) { double* d = a.position + 3 * (size_t)q; d[0] = P.x; d[1] = P.y; d[2] = P.z; }
    if (a.normal) { double* d = a.normal + 3 * (size_t)q; d[0] = N.x; d[1] = N.y; d[2] = N.z; }
    if (a.tri) a.tri[q] = owned ? (int32_t)t : -1;
    if (a.covered) a.covered[q] = owned ? 1 : 0;
}

hipError_t pt_chart_launch(const PtChartArgs& a, int which, hipStream_t stream) {
    const uint32_t n = a.width * a.height;  // (<= PT_AO_MAX = 2^24)
    if (which & 1) {
        hipLaunchKernelGGL(pt_chart_seed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, a.owner);
        if (a.n_tris) {
            const uint32_t map_tiles = ((a.width + PT_CHART_TILE - 1u) / PT_CHART_TILE) * ((a.height + PT_CHART_TILE - 1u) / PT_CHART_TILE);
            const uint32_t split = std::min<uint32_t>(std::min<uint32_t>(std::max<uint32_t>(PT_CHART_WAVES / a.n_tris, 1u), map_tiles), 65535u);
            hipLaunchKernelGGL(pt_chart_own_kernel, dim3((a.n_tris + 3u) / 4u, split), dim3(256), 0, stream, a);
        }
    }
    if (which & 2) hipLaunchKernelGGL(pt_chart_resolve_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// The contract on the host (no GPU, no context): what the three kernels do, by the functions they compile, in a fixed order - triangles ascending, so the first
// to cover a texel keeps it.
extern "C" int pt_test_chart_host(const double* fwd, const double* nrm, uint64_t n_tris, const double* tri_v, const double* tri_n, const double* uv, uint32_t width,
                                  uint32_t height, uint32_t flags, const pt_chart_buffers* out) {
    if (!fwd || !nrm || !out || (n_tris && (!tri_v || !uv))) return PT_ERR_ARGUMENT;
    if (!(out->position || out->normal || out->tri || out->covered)) return PT_ERR_ARGUMENT;
    if (width == 0 || height == 0 || (uint64_t)width * height > PT_AO_MAX || n_tris >= PT_CHART_NONE || (flags & ~PT_CHART_FLIP_NORMAL)) return PT_ERR_ARGUMENT;
    const size_t n = (size_t)width * height;
    std::vector<uint32_t> owner(n, PT_CHART_NONE);
    for (uint64_t t = 0; t < n_tris; t++) {
        double st[6], o, wt[4];
        int32_t x0, y0, x1, y1;
        if (!pt_chart_corners(uv + 6 * t, width, height, st) || !pt_chart_orientation(st, &o) || !pt_chart_box(st, width, height, &x0, &y0, &x1, &y1)) continue;
        for (int32_t y = y0; y <= y1; y++)
            for (int32_t x = x0; x <= x1; x++) {
                uint32_t& w = owner[(size_t)y * width + x];
                if (w == PT_CHART_NONE && pt_chart_covers(st, o, (double)x + 0.5, (double)y + 0.5, wt)) w = (uint32_t)t;
            }
    }
    for (size_t q = 0; q < n; q++) {
        const uint32_t t = owner[q];
        PtVec3 P = pt_v3(0.0, 0.0, 0.0), N = P;
        if (t != PT_CHART_NONE) {
            double st[6], o, wt[4];
            pt_chart_corners(uv + 6 * (size_t)t, width, height, st);
            pt_chart_orientation(st, &o);
            pt_chart_covers(st, o, (double)(q % width) + 0.5, (double)(q / width) + 0.5, wt);
            PtVec3 p, nm;
            pt_chart_surface(tri_v + 9 * (size_t)t, tri_n ? tri_n + 9 * (size_t)t : nullptr, wt, &p, &nm);
            pt_chart_world(fwd, nrm, flags, p, nm, &P, &N);
        }
        if (out->position) { out->position[3 * q] = P.x; out->position[3 * q + 1] = P.y; out->position[3 * q + 2] = P.z; }
        if (out->normal) { out->normal[3 * q] = N.x; out->normal[3 * q + 1] = N.y; out->normal[3 * q + 2] = N.z; }
        if (out->tri) out->tri[q] = t == PT_CHART_NONE ? -1 : (int32_t)t;
        if (out->covered) out->covered[q] = t == PT_CHART_NONE ? 0 : 1;
    }
    return PT_OK;
}
