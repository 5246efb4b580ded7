// The small kernels of the film's per-pixel budget (pt_film_add_map, pt_film_error, pt_film_budget_device: include/portrayer_hip.h) and their
// host-side replays: the PLAN that turns a budget map into the list the sampling kernel (pt_film_map.h) walks, the FOLD behind that kernel, the noise
// estimate and the budget a refine pass gives.
//
// The plan is an exclusive prefix sum of m_r over the pixel slots, written as separate kernels so that no block ever waits on another: block sums
// (count / reduce, one level per factor of PT_FILM_PLAN_BLOCK), a scan of the sums from the top level down, and the scatter that repeats the first level's
// block scan and writes the entries. The stream orders the kernels; inside a block only __syncthreads. No look-back, no spinning.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/portrayer_hip.h"
#include "pt_film_map_inst.h"
#include "pt_shade.h"

#define PT_PLAN_B PT_FILM_PLAN_BLOCK

// Exclusive scan of one value per thread over the block (Hillis-Steele in LDS); *block_total = the block's sum, for every thread.
static __device__ uint32_t pt_plan_block_scan(uint32_t v, uint32_t* block_total) {
    __shared__ uint32_t buf[2][PT_PLAN_B];
    const uint32_t t = threadIdx.x;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < PT_PLAN_B; d <<= 1) {
        buf[cur ^ 1][t] = t >= d ? buf[cur][t] + buf[cur][t - d] : buf[cur][t];
        cur ^= 1;
        __syncthreads();
    }
    const uint32_t incl = buf[cur][t];
    *block_total = buf[cur][PT_PLAN_B - 1];
    __syncthreads();  // (the buffer is free again for the caller's next scan)
    return incl - v;
}

// Level 0 -> 1: sums[b] = the samples of round `round` that block b's PT_PLAN_B slots want.
__global__ void __launch_bounds__(PT_PLAN_B) pt_film_plan_count_kernel(PtRenderArgs r, const uint32_t* __restrict__ budget, uint32_t max_samples, uint32_t round, uint32_t* __restrict__ sums) {
    size_t p;
    const uint32_t m = pt_film_map_slot_round(r, budget, max_samples, round, blockIdx.x * PT_PLAN_B + threadIdx.x, &p);
    uint32_t total;
    pt_plan_block_scan(m, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Level k -> k + 1: out[b] = the sum of block b's PT_PLAN_B words of in[0 .. n).
__global__ void __launch_bounds__(PT_PLAN_B) pt_film_plan_reduce_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * PT_PLAN_B + threadIdx.x;
    uint32_t total;
    pt_plan_block_scan(i < n ? in[i] : 0u, &total);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// data[0 .. n) -> its exclusive scan, block by block, every block starting at above[block] (the level above, already scanned); the top level is one block,
// has nothing above it and writes the grand total to *total_out.
__global__ void __launch_bounds__(PT_PLAN_B) pt_film_plan_scan_kernel(uint32_t* __restrict__ data, uint32_t n, const uint32_t* __restrict__ above, uint32_t* __restrict__ total_out) {
    const uint32_t i = blockIdx.x * PT_PLAN_B + threadIdx.x;
    uint32_t total;
    const uint32_t ex = pt_plan_block_scan(i < n ? data[i] : 0u, &total);
    if (i < n) data[i] = ex + (above ? above[blockIdx.x] : 0u);
    if (total_out && threadIdx.x == 0) *total_out = total;
}

// Level 0 again: every slot's offset = its block's (sums, scanned) + its place in the block; the slot writes its m_r entries there.
__global__ void __launch_bounds__(PT_PLAN_B) pt_film_plan_scatter_kernel(PtRenderArgs r, const uint32_t* __restrict__ budget, uint32_t max_samples, uint32_t round, const uint32_t* __restrict__ sums,
                                                                        uint32_t* __restrict__ list) {
    const uint32_t slot = blockIdx.x * PT_PLAN_B + threadIdx.x;
    size_t p;
    const uint32_t m = pt_film_map_slot_round(r, budget, max_samples, round, slot, &p);  // (<= PT_FILM_LW; 0 at and past n_slots)
    uint32_t total;
    const uint32_t at = sums[blockIdx.x] + pt_plan_block_scan(m, &total);  // (at + m <= the sum over all slots <= n_slots * PT_FILM_LW: the list's room)
    for (uint32_t j = 0; j < m; j++) list[at + j] = pt_film_map_entry(slot, j);
}

// One thread per pixel slot of the slice: the slot's m_r staged samples in ascending order, into total / partial, into q where the film has one.
__global__ void __launch_bounds__(256) pt_film_fold_map_kernel(PtFilmArgs a, const uint32_t* __restrict__ budget, uint32_t max_samples, uint32_t round, double* __restrict__ total,
                                                              double* __restrict__ partial, uint32_t* __restrict__ count, double* __restrict__ q2) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    size_t p;
    const uint32_t m = pt_film_map_slot_round(a.r, budget, max_samples, round, slot, &p);
    if (m == 0u) return;
    const uint32_t c = count[p];
    double *t = total + 3 * p, *q = partial + 3 * p;
    PtVec3 tot = pt_v3(t[0], t[1], t[2]), par = pt_v3(q[0], q[1], q[2]);
    double mom = q2 ? q2[p] : 0.0;
    const double* s = a.staging + 3 * (size_t)slot * a.lw;
    for (uint32_t j = 0; j < m; j++) {
        const PtVec3 v = pt_v3(s[3 * j], s[3 * j + 1], s[3 * j + 2]);
        pt_film_fold(tot, par, c + j, v);
        mom = pt_film_moment(mom, c + j, v);
    }
    t[0] = tot.x; t[1] = tot.y; t[2] = tot.z;
    q[0] = par.x; q[1] = par.y; q[2] = par.z;
    if (q2) q2[p] = mom;
    count[p] = c + m;
}

// One thread per pixel of the image.
__global__ void __launch_bounds__(256) pt_film_error_kernel(uint32_t n_pixels, const double* __restrict__ total, const double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                           const double* __restrict__ q2, double* __restrict__ err) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pixels) return;
    const double *t = total + 3 * (size_t)p, *q = partial + 3 * (size_t)p;
    err[p] = pt_film_error_of(pt_v3(t[0], t[1], t[2]), pt_v3(q[0], q[1], q[2]), q2[p], count[p]);
}

// What a refine pass gives a pixel with count c and error e (pt_film_budget_device).
PT_HD uint32_t pt_film_budget_of(uint32_t c, double e, double threshold, uint32_t min_count, uint32_t max_count, uint32_t step) {
    if (c < min_count) return min_count - c < step ? min_count - c : step;
    if (c < max_count && e > threshold) return step < max_count - c ? step : max_count - c;
    return 0u;
}

// One thread per pixel of the image: 0 outside the slice. The summary: one pair of atomics per wavefront that has anything to report.
__global__ void __launch_bounds__(256) pt_film_budget_kernel(PtRenderArgs r, double threshold, uint32_t min_count, uint32_t max_count, uint32_t step, const double* __restrict__ total,
                                                            const double* __restrict__ partial, const uint32_t* __restrict__ count, const double* __restrict__ q2, uint32_t* __restrict__ budget,
                                                            unsigned long long* __restrict__ summary) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t b = 0;
    if (p < r.width * r.height) {
        const uint32_t x = p % r.width, y = p / r.width;
        if (x >= r.x0 && x <= r.x1 && y >= r.y0 && y <= r.y1) {
            const double *t = total + 3 * (size_t)p, *q = partial + 3 * (size_t)p;
            const uint32_t c = count[p];
            b = pt_film_budget_of(c, pt_film_error_of(pt_v3(t[0], t[1], t[2]), pt_v3(q[0], q[1], q[2]), q2[p], c), threshold, min_count, max_count, step);
        }
        budget[p] = b;
    }
    const unsigned long long wanting = __ballot(b > 0u);
    if (wanting == 0ull) return;  // (the whole wavefront)
    uint32_t sum = b;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(summary, (unsigned long long)__popcll(wanting));
        atomicAdd(summary + 1, (unsigned long long)sum);
    }
}

// The scan's levels: n[0] = blocks of slots, n[k + 1] = blocks of n[k] words, down to one block. Returns the number of levels (>= 1), at most 4 below 2^29 slots.
static int pt_film_plan_levels(uint32_t n_slots, uint32_t n[4]) {
    int levels = 0;
    uint32_t k = n_slots;
    do {
        k = (k + PT_PLAN_B - 1u) / PT_PLAN_B;
        n[levels++] = k;
    } while (k > PT_PLAN_B && levels < 4);
    return levels;
}

size_t pt_film_plan_words(uint32_t n_slots) {
    uint32_t n[4];
    const int levels = pt_film_plan_levels(n_slots, n);
    size_t words = 0;
    for (int k = 0; k < levels; k++) words += n[k];
    return words;
}

hipError_t pt_film_plan_launch(const PtRenderArgs& r, const uint32_t* budget, uint32_t max_samples, uint32_t round, uint32_t* work, uint32_t* list, uint32_t* n_list, hipStream_t stream) {
    if (r.n_slots == 0) return hipMemsetAsync(n_list, 0, 4, stream);
    uint32_t n[4];
    const int levels = pt_film_plan_levels(r.n_slots, n);
    uint32_t* sums[4];
    for (int k = 0; k < levels; k++) { sums[k] = work; work += n[k]; }
    hipLaunchKernelGGL(pt_film_plan_count_kernel, dim3(n[0]), dim3(PT_PLAN_B), 0, stream, r, budget, max_samples, round, sums[0]);
    for (int k = 1; k < levels; k++) hipLaunchKernelGGL(pt_film_plan_reduce_kernel, dim3(n[k]), dim3(PT_PLAN_B), 0, stream, (const uint32_t*)sums[k - 1], n[k - 1], sums[k]);
    // from the top (one block: n[levels - 1] <= PT_PLAN_B words) down
    for (int k = levels - 1; k >= 0; k--) {
        const bool top = k == levels - 1;
        hipLaunchKernelGGL(pt_film_plan_scan_kernel, dim3(top ? 1u : n[k + 1]), dim3(PT_PLAN_B), 0, stream, sums[k], n[k], top ? (const uint32_t*)nullptr : (const uint32_t*)sums[k + 1],
                           top ? n_list : (uint32_t*)nullptr);
    }
    hipLaunchKernelGGL(pt_film_plan_scatter_kernel, dim3(n[0]), dim3(PT_PLAN_B), 0, stream, r, budget, max_samples, round, (const uint32_t*)sums[0], list);
    return hipGetLastError();
}

hipError_t pt_film_fold_map_launch(const PtFilmArgs& a, const uint32_t* budget, uint32_t max_samples, uint32_t round, double* total, double* partial, uint32_t* count, double* q, hipStream_t stream) {
    if (a.r.n_slots == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_film_fold_map_kernel, dim3((a.r.n_slots + 255u) / 256u), dim3(256), 0, stream, a, budget, max_samples, round, total, partial, count, q);
    return hipGetLastError();
}

hipError_t pt_film_error_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, double* err, hipStream_t stream) {
    const uint32_t n = width * height;  // (pt_film_create refuses films of 2^31 pixels or more)
    hipLaunchKernelGGL(pt_film_error_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, total, partial, count, q, err);
    return hipGetLastError();
}

hipError_t pt_film_budget_launch(const PtRenderArgs& r, double threshold, uint32_t min_count, uint32_t max_count, uint32_t step, const double* total, const double* partial, const uint32_t* count,
                                 const double* q, uint32_t* budget, unsigned long long* summary, hipStream_t stream) {
    const uint32_t n = r.width * r.height;
    hipLaunchKernelGGL(pt_film_budget_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, r, threshold, min_count, max_count, step, total, partial, count, q, budget, summary);
    return hipGetLastError();
}

// The slice of a width-wide image as the kernels see it (pt_fill_args fills the same fields for a pass).
static void pt_film_map_host_slice(uint32_t width, uint32_t height, const pt_rect* slice, PtRenderArgs* r) {
    memset(r, 0, sizeof *r);
    r->width = width; r->height = height;
    r->x0 = slice->x0; r->y0 = slice->y0; r->x1 = slice->x1; r->y1 = slice->y1;
    r->tile_rank = 0; r->tile_ranks = 1;
    const uint64_t tiles = (uint64_t)((slice->x1 - slice->x0 + 8u) / 8u) * ((slice->y1 - slice->y0 + 8u) / 8u);
    r->n_slots = (uint32_t)(tiles * 64u);
}

// Host-side replay (no GPU, no context) of the plan of round `round`: the list the plan kernels write, by the functions they call. *n_out = its length, also
// where it exceeds `cap` (then only `cap` entries are written).
extern "C" int pt_test_film_plan_host(uint32_t width, uint32_t height, const pt_rect* slice, const uint32_t* budget, uint32_t max_samples, uint32_t round, uint32_t* list, uint32_t cap,
                                      uint32_t* n_out) {
    if (!slice || !budget || !n_out || (!list && cap) || width == 0 || height == 0 || max_samples == 0 || max_samples > PT_FILM_MAP_MAX) return PT_ERR_ARGUMENT;
    if (round >= (PT_FILM_MAP_MAX + PT_FILM_LW - 1) / PT_FILM_LW) return PT_ERR_ARGUMENT;
    if (slice->x0 > slice->x1 || slice->y0 > slice->y1 || slice->x1 >= width || slice->y1 >= height) return PT_ERR_SLICE;
    if ((uint64_t)((slice->x1 - slice->x0 + 8u) / 8u) * ((slice->y1 - slice->y0 + 8u) / 8u) * 64u >= PT_FILM_MAP_SLOTS_MAX) return PT_ERR_ARGUMENT;
    PtRenderArgs r;
    pt_film_map_host_slice(width, height, slice, &r);
    uint64_t n = 0;
    for (uint32_t slot = 0; slot < r.n_slots; slot++) {
        size_t p;
        const uint32_t m = pt_film_map_slot_round(r, budget, max_samples, round, slot, &p);
        for (uint32_t j = 0; j < m; j++, n++)
            if (n < cap) list[n] = pt_film_map_entry(slot, j);
    }
    *n_out = (uint32_t)n;
    return PT_OK;
}

// Host-side replay (no GPU, no context) of a film with moments at one pixel: n samples in n_cuts consecutive adds of cuts[k] samples each, every add split
// into rounds of at most PT_FILM_LW and folded as pt_film_fold_map_kernel folds them; out_sum = what resolve divides, out_q the second moment, out_err what
// pt_film_error writes. n = 0 (no cuts): out_err alone, +inf.
extern "C" int pt_test_film_moments_host(uint32_t n, const double* samples, const uint32_t* cuts, uint32_t n_cuts, double out_sum[3], double* out_q, double* out_err) {
    if (!out_sum || !out_q || !out_err || (n && (!samples || !cuts || n_cuts == 0))) return PT_ERR_ARGUMENT;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_cuts && n; k++) sum += cuts[k];
    if (sum != n) return PT_ERR_ARGUMENT;
    PtVec3 tot = pt_v3(0.0, 0.0, 0.0), par = pt_v3(0.0, 0.0, 0.0);
    double mom = 0.0;
    uint32_t count = 0;
    for (uint32_t k = 0; k < n_cuts && n; k++)
        for (uint32_t round = 0;; round++) {
            const uint32_t m = pt_film_map_round(cuts[k], cuts[k], round);
            if (m == 0u) break;
            const double* s = samples + 3 * (size_t)count;
            for (uint32_t j = 0; j < m; j++) {
                const PtVec3 v = pt_v3(s[3 * j], s[3 * j + 1], s[3 * j + 2]);
                pt_film_fold(tot, par, count + j, v);
                mom = pt_film_moment(mom, count + j, v);
            }
            count += m;
        }
    const PtVec3 r = count ? pt_film_sum(tot, par, count) : pt_v3(0.0, 0.0, 0.0);
    out_sum[0] = r.x; out_sum[1] = r.y; out_sum[2] = r.z;
    *out_q = mom;
    *out_err = pt_film_error_of(tot, par, mom, count);
    return PT_OK;
}
