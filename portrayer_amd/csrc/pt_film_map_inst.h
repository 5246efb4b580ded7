// The film's per-pixel budget (pt_film_add_map, include/portrayer_hip.h): the argument block of the list-driven sampling kernel (pt_film_map.h),
// the functions that say what a pixel gets in a launch round and how a sample is named in the list - shared by the plan kernels, the fold kernel and the
// host replay (pt_film_map.hip) - the second moment and the error estimate, and the launchers: one per traversal mode for the sampling kernel, each in its
// own object (pt_film_map_inst.hip compiled with -DPT_INST_MODE=<mode>), and the small kernels' (pt_film_map.hip).
#pragma once

#include "pt_film_inst.h"

// An entry of the list is one u32: the sample's place in the staging buffer, slot * PT_FILM_LW + j. Slices of 2^29 slots or more are refused.
#define PT_FILM_MAP_LW_LOG2 3
static_assert((1 << PT_FILM_MAP_LW_LOG2) == PT_FILM_LW, "a list entry is slot << 3 | j");
#define PT_FILM_MAP_SLOTS_MAX 0x20000000u
#define PT_FILM_PLAN_BLOCK 256  // slots (and block sums) per block of the plan kernels: one level of the scan per factor of 256

struct PtFilmMapArgs {
    PtFilmArgs f;            // FIRST (the kernel re-reads the block through the kernarg segment). f.r.n_items: the HOST's upper bound of the list's wavefronts;
                             // f.launch_samples, f.k_log2 unused; f.lw = PT_FILM_LW
    const uint32_t* list;    // one entry per sample of this round, ascending (slot, j)
    const uint32_t* n_list;  // the list's length, a device word written by the plan
};
static_assert(offsetof(PtFilmMapArgs, f) == 0, "the kernel reads PtRenderArgs at the start of its argument block");

// What the map gives a pixel in all (m) and in launch round r (m_r): the next min(budget, max_samples) samples, PT_FILM_LW per round.
PT_HD uint32_t pt_film_map_round(uint32_t budget, uint32_t max_samples, uint32_t round) {
    const uint32_t m = budget < max_samples ? budget : max_samples;
    const uint32_t done = round * (uint32_t)PT_FILM_LW;  // (round < PT_FILM_MAP_MAX / PT_FILM_LW)
    if (m <= done) return 0u;
    return m - done < (uint32_t)PT_FILM_LW ? m - done : (uint32_t)PT_FILM_LW;
}
// ... of pixel slot `slot` of the slice (0 outside it). budget == nullptr: a uniform add of `max_samples` (pt_film_add on a film with moments).
PT_HD uint32_t pt_film_map_slot_round(const PtRenderArgs& r, const uint32_t* budget, uint32_t max_samples, uint32_t round, uint32_t slot, size_t* pixel) {
    uint32_t x, y;
    *pixel = 0;
    if (slot >= r.n_slots || !pt_slot_to_pixel(r, slot, &x, &y)) return 0u;
    *pixel = (size_t)y * r.width + x;
    return pt_film_map_round(budget ? budget[*pixel] : max_samples, max_samples, round);
}
PT_HD uint32_t pt_film_map_entry(uint32_t slot, uint32_t j) { return (slot << PT_FILM_MAP_LW_LOG2) | j; }

// The second moment of a film with moments: sample s of a pixel, value v. Plain ascending order, no chunks: the first sample is assigned.
PT_HD double pt_film_moment(double q, uint32_t s, PtVec3 v) {
    const double y = (v.x + v.y) + v.z;
    const double yy = y * y;
    return s == 0u ? yy : q + yy;
}
// The standard error of the mean of the channel sum out of a pixel's state, in exactly this order of operations (include/portrayer_hip.h).
PT_HD double pt_film_error_of(PtVec3 total, PtVec3 partial, double q, uint32_t n) {
    if (n < 2u) return INFINITY;
    const PtVec3 S = pt_film_sum(total, partial, n);
    const double dn = (double)n;
    const PtVec3 mean = S / dn;
    const double my = (mean.x + mean.y) + mean.z;
    double var = (q - (dn * my) * my) / (double)(n - 1u);
    if (!(var > 0.0)) var = 0.0;
    return sqrt(var / dn);
}

PT_DECLARE_MODE_LAUNCHERS(pt_film_map_launch_mode_, const PtFilmMapArgs& a, bool tex, bool park, int n_cu, hipStream_t stream, uint32_t* grid, bool launch);

// pt_film_map.hip. All take the slice / image through PtRenderArgs' fields (width, height, x0 .. y1, n_slots) and queue their kernels on `stream`.
// Words of work space the plan of a slice of n_slots needs (the block sums of every level of the scan).
size_t pt_film_plan_words(uint32_t n_slots);
// plan: round `round` of the map -> list (one entry per sample, ascending (slot, j); room for n_slots * PT_FILM_LW) and its length in *n_list.
// budget == nullptr: max_samples for every pixel of the slice.
hipError_t pt_film_plan_launch(const PtRenderArgs& r, const uint32_t* budget, uint32_t max_samples, uint32_t round, uint32_t* work, uint32_t* list, uint32_t* n_list, hipStream_t stream);
// fold: one thread per pixel slot; the slot's m_r staged samples (a.staging, a.lw) folded in ascending order, q likewise where the film has one (q may be
// null), count += m_r.
hipError_t pt_film_fold_map_launch(const PtFilmArgs& a, const uint32_t* budget, uint32_t max_samples, uint32_t round, double* total, double* partial, uint32_t* count, double* q, hipStream_t stream);
// error: one thread per pixel of the image, err = pt_film_error_of.
hipError_t pt_film_error_launch(uint32_t width, uint32_t height, const double* total, const double* partial, const uint32_t* count, const double* q, double* err, hipStream_t stream);
// budget: one thread per pixel of the image (pt_film_budget_device); summary[0] += pixels with a budget, summary[1] += their budgets (the caller zeroes it).
hipError_t pt_film_budget_launch(const PtRenderArgs& r, double threshold, uint32_t min_count, uint32_t max_count, uint32_t step, const double* total, const double* partial, const uint32_t* count,
                                 const double* q, uint32_t* budget, unsigned long long* summary, hipStream_t stream);
